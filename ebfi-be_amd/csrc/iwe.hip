// The event-warping losses of loss/flow.py and myutils/iwe.py on the device: get_interpolation, interpolate, deblur_events /
// compute_pol_iwe, the contrast-maximisation loss EventWarping (forward and the gradient into the flow) and AveragedIWE.
//
// THE LAW.  interpolate is a scatter_add_ along dim 1 of fractional fp32 weights; with one thread it walks the list serially,
// so every pixel receives its addends in ASCENDING LIST POSITION, each product and sum its own fp32 rounding.  As in
// csrc/encodings.hip the scatter becomes a gather: a key per list entry (b * H * W + idx; unfeasible or out-of-range entries
// take the unread key B * H * W), a stable 8-bit LSD radix sort of (key, position), run starts by bisection, then one thread
// per pixel that adds its run in order, every plane its own chain of adds over one shared gather; a run of 64 entries or more
// is gathered by the whole wave and summed over the lanes in lane order.  No float atomics, nothing read back, every launch on the caller's stream in one chain.
// The gradient of EventWarping is a gather too: the events are sorted once by SOURCE pixel (independent of the flow), one
// thread per source pixel walks its run in event order and writes each flow element once.
//
// The sort is a private copy of the one in csrc/encodings.hip (tests/test_encodings_host.py counts that file's launches, so the
// kernels could not move into a shared header without touching it; DESIGN.md says so).
#include "common.hpp"

#pragma clang fp contract(off)

using namespace ebfi;

namespace {

constexpr int kBlock = 256;
constexpr int kScanTile = 1024;
constexpr uint32_t kLongRun = 64;

// ------------------------------------------------------------------ stable LSD radix sort, 8 bits per pass (as encodings.hip)
__global__ void sort_hist(const uint32_t *__restrict__ keys, int64_t n, int shift, uint32_t *__restrict__ hist, int nb) {
    __shared__ uint32_t h[256];
    h[threadIdx.x] = 0;
    __syncthreads();
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i < n) atomicAdd(&h[(keys[i] >> shift) & 255u], 1u);
    __syncthreads();
    hist[(int64_t)threadIdx.x * nb + blockIdx.x] = h[threadIdx.x];
}

__device__ __forceinline__ uint32_t block_exclusive_scan(uint32_t v, uint32_t *buf /* [256] */, uint32_t *total) {
    const int t = threadIdx.x;
    buf[t] = v;
    __syncthreads();
    for (int d = 1; d < kBlock; d <<= 1) {
        const uint32_t add = t >= d ? buf[t - d] : 0u;
        __syncthreads();
        buf[t] += add;
        __syncthreads();
    }
    const uint32_t incl = buf[t];
    *total = buf[kBlock - 1];
    __syncthreads();
    return incl - v;
}

__global__ void scan_tiles(uint32_t *__restrict__ table, int64_t m, uint32_t *__restrict__ sums) {
    __shared__ uint32_t buf[kBlock];
    const int64_t base = (int64_t)blockIdx.x * kScanTile + (int64_t)threadIdx.x * 4;
    uint32_t v[4], s = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        v[k] = base + k < m ? table[base + k] : 0u;
        s += v[k];
    }
    uint32_t total;
    uint32_t pre = block_exclusive_scan(s, buf, &total);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (base + k < m) table[base + k] = pre;
        pre += v[k];
    }
    if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

__global__ void scan_sums(uint32_t *__restrict__ sums, int64_t nt) {
    __shared__ uint32_t buf[kBlock];
    uint32_t carry = 0;
    for (int64_t base = 0; base < nt; base += kBlock) {
        const int64_t i = base + threadIdx.x;
        const uint32_t v = i < nt ? sums[i] : 0u;
        uint32_t total;
        const uint32_t pre = block_exclusive_scan(v, buf, &total);
        if (i < nt) sums[i] = carry + pre;
        carry += total;
    }
}

// perm_in == nullptr: the permutation so far is the identity
__global__ void sort_scatter(const uint32_t *__restrict__ keys_in, const uint32_t *__restrict__ perm_in, int64_t n, int shift,
                             const uint32_t *__restrict__ hist, const uint32_t *__restrict__ sums, int nb,
                             uint32_t *__restrict__ keys_out, uint32_t *__restrict__ perm_out) {
    __shared__ uint32_t wcnt[kBlock / 64][256];
    for (int k = threadIdx.x; k < (kBlock / 64) * 256; k += kBlock) (&wcnt[0][0])[k] = 0;
    __syncthreads();
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const bool active = i < n;
    const uint32_t key = active ? keys_in[i] : 0u;
    const uint32_t d = (key >> shift) & 255u;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned long long same = __ballot(active);
#pragma unroll
    for (int b = 0; b < 8; ++b) {
        const bool bit = (d >> b) & 1u;
        const unsigned long long bal = __ballot(active && bit);
        same &= bit ? bal : ~bal;
    }
    const uint32_t rank = (uint32_t)__popcll(same & ((1ull << lane) - 1ull));
    if (active && rank == 0) wcnt[wave][d] = (uint32_t)__popcll(same);
    __syncthreads();
    if (!active) return;
    const int64_t slot = (int64_t)d * nb + blockIdx.x;
    uint32_t at = hist[slot] + sums[slot / kScanTile] + rank;
    for (int w = 0; w < wave; ++w) at += wcnt[w][d];
    keys_out[at] = key;                  // at < n: the table counts exactly the n active entries
    perm_out[at] = perm_in ? perm_in[i] : (uint32_t)i;
}

// seg[k] = first position of the sorted keys that is >= k, for k in [0, nkeys]
__global__ void run_starts(const uint32_t *__restrict__ keys, int64_t n, int64_t nkeys, uint32_t *__restrict__ seg) {
    const int64_t k = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (k > nkeys) return;
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        const int64_t mid = lo + (hi - lo) / 2;
        if ((int64_t)keys[mid] < k) lo = mid + 1;
        else hi = mid;
    }
    seg[k] = (uint32_t)lo;
}

// keys_out[j] = table[perm[j]]: the keys of the next, more significant sort in the order of the previous one (no perm: a copy)
__global__ void gather_keys(const uint32_t *__restrict__ table, const uint32_t *__restrict__ perm, int64_t n,
                            uint32_t *__restrict__ keys_out) {
    const int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (j < n) keys_out[j] = table[perm ? perm[j] : (uint32_t)j];
}

// ------------------------------------------------------------------ the warp of one event
struct Flow4 {
    const float *p;
    int64_t sb, sc, sh, sw;      // strides in elements
};

// source pixel of an event: integral coordinates inside the image, else -1 (the reference's gather raises there)
__device__ __forceinline__ int64_t source_pixel(float y, float x, int H, int W) {
    if (!(y >= 0.f && y < (float)H && x >= 0.f && x < (float)W)) return -1;
    if (y != floorf(y) || x != floorf(x)) return -1;
    return (int64_t)y * W + (int64_t)x;
}

// warped position: pos + (((tref - ts) * flow) * scaling), fp32, in that order
__device__ __forceinline__ float warp1(float pos, float ts, float f, float tref, float scaling) {
    return pos + (((tref - ts) * f) * scaling);
}

struct Corner {
    float cy, cx;      // integer corner coordinates (as floats)
    float ay, ax;      // per-axis weights max(0, 1 - |warped - corner|)
    bool ok;           // feasible and finite
};

__device__ __forceinline__ Corner corner_of(float wy, float wx, int c, int round_idx, int H, int W) {
    Corner k;
    if (round_idx) {
        k.cy = rintf(wy);      // torch.round: half to even
        k.cx = rintf(wx);
        k.ay = 1.f;
        k.ax = 1.f;
    } else {
        k.cy = (c >> 1) ? floorf(wy + 1.f) : floorf(wy);
        k.cx = (c & 1) ? floorf(wx + 1.f) : floorf(wx);
        k.ay = fmaxf(0.f, 1.f - fabsf(wy - k.cy));
        k.ax = fmaxf(0.f, 1.f - fabsf(wx - k.cx));
    }
    // a NaN or infinite coordinate fails one of the comparisons or gives a non-finite corner: weight 0
    k.ok = k.cy >= 0.f && k.cy < (float)H && k.cx >= 0.f && k.cx < (float)W && wy - wy == 0.f && wx - wx == 0.f;
    return k;
}

// One thread per event: its corners' float index, weight and sort key.  flow_ev [B, N, 2] = (y, x) per event, or the flow map
// (gathered at the source pixel; an event whose source is outside the image or not integral takes flow 0 and weight 0).
// idx / weights [B, M] with M = corners * N, corner-major (the reference concatenates the four corner lists along N);
// keys [B * M] (optional): b * P + idx, or B * P for weight-less entries; src / pol (optional, AveragedIWE): per event.
__global__ void warp_events(const float *__restrict__ events, const float *__restrict__ flow_ev, Flow4 flow, int64_t B, int64_t N,
                            float tref, float scaling, int round_idx, int H, int W, float *__restrict__ idx,
                            float *__restrict__ weights, uint32_t *__restrict__ keys, uint32_t *__restrict__ src_keys,
                            uint32_t *__restrict__ pol_keys) {
    const int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (e >= B * N) return;
    const int64_t b = e / N, n = e % N, P = (int64_t)H * W;
    const float ts = events[e * 4], y = events[e * 4 + 1], x = events[e * 4 + 2];
    float fy, fx;
    bool src_ok = true;
    int64_t src = -1;
    if (flow_ev) {
        fy = flow_ev[e * 2];
        fx = flow_ev[e * 2 + 1];
    } else {
        src = source_pixel(y, x, H, W);
        src_ok = src >= 0;
        fy = fx = 0.f;
        if (src_ok) {
            const int64_t at = b * flow.sb + (src / W) * flow.sh + (src % W) * flow.sw;
            fy = flow.p[at + flow.sc];      // channel 1: the vertical component
            fx = flow.p[at];
        }
    }
    const float wy = warp1(y, ts, fy, tref, scaling), wx = warp1(x, ts, fx, tref, scaling);
    const int corners = round_idx ? 1 : 4;
    const int64_t M = corners * N;
    bool any = false;
    for (int c = 0; c < corners; ++c) {
        const Corner k = corner_of(wy, wx, c, round_idx, H, W);
        const bool ok = k.ok && src_ok;
        const float fi = ok ? k.cy * (float)W + k.cx : 0.f;
        const float w = ok ? k.ay * k.ax : 0.f;
        const int64_t g = b * M + (int64_t)c * N + n;
        if (idx) idx[g] = fi;
        if (weights) weights[g] = w;
        if (keys) {
            const int64_t pix = (int64_t)fi;
            keys[g] = (ok && pix >= 0 && pix < P) ? (uint32_t)(b * P + pix) : (uint32_t)(B * P);
        }
        any = any || (ok && w != 0.f);
    }
    if (src_keys) {      // AveragedIWE: `p < 1` is negative; weight 0 marks an unfeasible mapping (fake polarity 2)
        src_keys[e] = src_ok ? (uint32_t)(b * P + src) : (uint32_t)(B * P);
        pol_keys[e] = any ? (events[e * 4 + 3] < 1.f ? 0u : 1u) : 2u;
    }
}

// keys of the public interpolate(): idx float32 or int64 [B, M]; an index outside [0, H * W) is dropped (the reference raises)
__global__ void interpolate_keys(const void *__restrict__ idx, int idx_is_i64, int64_t B, int64_t M, int64_t P,
                                 uint32_t *__restrict__ keys) {
    const int64_t g = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (g >= B * M) return;
    int64_t pix = -1;
    if (idx_is_i64) {
        pix = static_cast<const int64_t *>(idx)[g];
    } else {
        const float f = static_cast<const float *>(idx)[g];
        if (f > -1.f && f < 4294967296.f) pix = (int64_t)f;      // .long(): truncation; a NaN fails both comparisons
    }
    keys[g] = (pix >= 0 && pix < P) ? (uint32_t)((g / M) * P + pix) : (uint32_t)(B * P);
}

// keys of the source-pixel index of the gradient: one per event
__global__ void source_keys(const float *__restrict__ events, int64_t B, int64_t N, int H, int W, uint32_t *__restrict__ keys) {
    const int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (e >= B * N) return;
    const int64_t P = (int64_t)H * W, src = source_pixel(events[e * 4 + 1], events[e * 4 + 2], H, W);
    keys[e] = src >= 0 ? (uint32_t)((e / N) * P + src) : (uint32_t)(B * P);
}

// ------------------------------------------------------------------ the ordered accumulation
// planes: 1 = weights * mask_a (a null mask leaves the weight as it is); 2 = (weights * mask_a, weights * mask_b); 4 = those
// two, then ((weights * t) * mask_a, (weights * t) * mask_b) with t = ts (tmode 1) or 1 - ts (tmode 2).
// Entry g = b * M + m belongs to event n = m % N (the masks and stamps repeat per corner).
struct AccArgs {
    const float *w, *mask_a, *mask_b, *events;
    int64_t mstride, N, M;
    int tmode;
};

// the addends of list entry g, one per plane: the entry, its stamp and its masks are read once for all planes
template <int PLANES>
__device__ __forceinline__ void addends(const AccArgs &a, uint32_t g, float *v) {
    const int64_t b = (int64_t)g / a.M, n = ((int64_t)g % a.M) % a.N, e = b * a.N + n;
    const float w = a.w[g];
    const float ma = a.mask_a ? a.mask_a[e * a.mstride] : 1.f;
    v[0] = a.mask_a ? w * ma : w;
    if (PLANES >= 2) {
        const float mb = a.mask_b[e * a.mstride];
        v[1] = w * mb;
        if (PLANES == 4) {
            float t = a.events[e * 4];
            if (a.tmode == 2) t = 1.f - t;
            const float wt = w * t;
            v[2] = wt * ma;
            v[3] = wt * mb;
        }
    }
}

// out [B, PLANES, P]; one thread per pixel key adds its run in list order, every plane its own chain; every element written
template <int PLANES>
__global__ void accumulate(AccArgs a, const uint32_t *__restrict__ perm, const uint32_t *__restrict__ seg, int64_t nkeys,
                           int64_t P, float *__restrict__ out) {
    const int64_t key = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const bool valid = key < nkeys;
    uint32_t s = 0, e = 0;
    if (valid) s = seg[key], e = seg[key + 1];
    float acc[PLANES];
#pragma unroll
    for (int p = 0; p < PLANES; ++p) acc[p] = 0.f;
    const bool is_long = e - s >= kLongRun;
    if (!is_long) {
        for (uint32_t j = s; j < e; ++j) {
            float v[PLANES];
            addends<PLANES>(a, perm[j], v);
#pragma unroll
            for (int p = 0; p < PLANES; ++p) acc[p] = acc[p] + v[p];
        }
    }
    const int lane = threadIdx.x & 63;
    unsigned long long todo = __ballot(is_long);
    while (todo) {
        const int owner = __ffsll((long long)todo) - 1;
        todo &= todo - 1;
        const uint32_t ls = (uint32_t)__shfl((int)s, owner), le = (uint32_t)__shfl((int)e, owner);
        float run[PLANES];
#pragma unroll
        for (int p = 0; p < PLANES; ++p) run[p] = 0.f;
        for (uint32_t j = ls; j < le; j += 64) {
            const uint32_t cnt = le - j < 64u ? le - j : 64u;
            float v[PLANES];
#pragma unroll
            for (int p = 0; p < PLANES; ++p) v[p] = 0.f;
            if ((uint32_t)lane < cnt) addends<PLANES>(a, perm[j + lane], v);
            for (uint32_t k = 0; k < cnt; ++k) {      // lane order == list order
#pragma unroll
                for (int p = 0; p < PLANES; ++p) run[p] = run[p] + __shfl(v[p], (int)k);
            }
        }
        if (lane == owner) {
#pragma unroll
            for (int p = 0; p < PLANES; ++p) acc[p] = run[p];
        }
    }
    if (!valid) return;
#pragma unroll
    for (int p = 0; p < PLANES; ++p) out[((key / P) * PLANES + p) * P + key % P] = acc[p];
}

// ------------------------------------------------------------------ EventWarping: the loss
// images [2 (fw, bw)][B][4 (count+, count-, stamp+, stamp-)][P].  Term i < 4 B P: the squared ratio of one (direction, item,
// polarity, pixel); term i < 2 B P also: weight * (charbonnier of the differences below and to the right of flow element i).
__device__ __forceinline__ double block_sum(double v, double *buf) {
    buf[threadIdx.x] = v;
    __syncthreads();
    for (int d = kBlock / 2; d > 0; d >>= 1) {
        if ((int)threadIdx.x < d) buf[threadIdx.x] = buf[threadIdx.x] + buf[threadIdx.x + d];
        __syncthreads();
    }
    return buf[0];
}

__global__ void loss_partials(const float *__restrict__ images, Flow4 flow, int64_t B, int H, int W, double weight,
                              double *__restrict__ partials) {
    __shared__ double buf[kBlock];
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x, P = (int64_t)H * W;
    double v = 0.0;
    if (i < 4 * B * P) {
        const int64_t pix = i % P, q = (i / P) % 2, b = (i / (2 * P)) % B, d = i / (2 * P * B);
        const float *img = images + ((d * B + b) * 4) * P;
        const float den = img[q * P + pix] + 1e-9f;
        const float r = img[(2 + q) * P + pix] / den;
        v = (double)r * (double)r;
    }
    if (i < 2 * B * P) {
        const int64_t pix = i % P, c = (i / P) % 2, b = i / (2 * P);
        const int h = (int)(pix / W), w = (int)(pix % W);
        const float *f = flow.p + b * flow.sb + c * flow.sc + h * flow.sh + w * flow.sw;
        double s = 0.0;
        if (h + 1 < H) {
            const float dd = f[0] - f[flow.sh];
            s = s + sqrt((double)dd * (double)dd + 1e-6);
        }
        if (w + 1 < W) {
            const float dd = f[0] - f[flow.sw];
            s = s + sqrt((double)dd * (double)dd + 1e-6);
        }
        v = v + weight * s;
    }
    const double total = block_sum(v, buf);
    if (threadIdx.x == 0) partials[blockIdx.x] = total;
}

__global__ void loss_final(const double *__restrict__ partials, int64_t n, float *__restrict__ loss) {
    __shared__ double buf[kBlock];
    double v = 0.0;
    for (int64_t i = threadIdx.x; i < n; i += kBlock) v = v + partials[i];
    const double total = block_sum(v, buf);
    if (threadIdx.x == 0) *loss = (float)total;
}

// ------------------------------------------------------------------ EventWarping: the gradient into the flow
struct BwdArgs {
    const float *events, *pol_mask, *images;
    Flow4 flow;
    int64_t B, N;
    int H, W;
    float scaling;
};

// d max(0, 1 - |u|) / du with torch's subgradients: abs'(0) = 0, a tie of the max passes half
__device__ __forceinline__ double tent_slope(float u) {
    const float a = 1.f - fabsf(u);
    const double sg = u > 0.f ? -1.0 : (u < 0.f ? 1.0 : 0.0);
    return a > 0.f ? sg : (a == 0.f ? 0.5 * sg : 0.0);
}

// what event e adds to d loss / d (fy, fx) of its source pixel: forward direction first, then backward; corners in order
__device__ __forceinline__ void event_gradient(const BwdArgs &a, int64_t e, float fy, float fx, double *gy, double *gx) {
    const int64_t b = e / a.N, P = (int64_t)a.H * a.W;
    const float ts = a.events[e * 4], y = a.events[e * 4 + 1], x = a.events[e * 4 + 2];
    const float pm[2] = {a.pol_mask[e * 2], a.pol_mask[e * 2 + 1]};
    double sy = 0.0, sx = 0.0;
    for (int d = 0; d < 2; ++d) {
        const float tref = d == 0 ? 1.f : 0.f;
        const float t = d == 0 ? ts : 1.f - ts;
        const float wy = warp1(y, ts, fy, tref, a.scaling), wx = warp1(x, ts, fx, tref, a.scaling);
        const double chain = (double)(tref - ts) * (double)a.scaling;
        const float *img = a.images + ((d * a.B + b) * 4) * P;
        for (int c = 0; c < 4; ++c) {
            const Corner k = corner_of(wy, wx, c, 0, a.H, a.W);
            if (!k.ok) continue;
            const int64_t pix = (int64_t)(k.cy * (float)a.W + k.cx);
            if (pix < 0 || pix >= P) continue;
            double gw = 0.0;      // d loss / d weight of this corner
            for (int q = 0; q < 2; ++q) {
                if (pm[q] == 0.f) continue;
                const float den = img[q * P + pix] + 1e-9f;
                const float r = img[(2 + q) * P + pix] / den;
                gw = gw + (double)pm[q] * (2.0 * (double)r * ((double)t - (double)r) / (double)den);
            }
            sy = sy + gw * (tent_slope(wy - k.cy) * (double)k.ax) * chain;
            sx = sx + gw * (tent_slope(wx - k.cx) * (double)k.ay) * chain;
        }
    }
    *gy = sy;
    *gx = sx;
}

// d (sum of charbonnier terms) / d f[h][w] of one channel: a gather from up to four neighbours
__device__ __forceinline__ double smooth_gradient(const float *f, int h, int w, int H, int W, int64_t sh, int64_t sw) {
    double g = 0.0;
    if (h + 1 < H) {
        const float d = f[0] - f[sh];
        g = g + (double)d / sqrt((double)d * (double)d + 1e-6);
    }
    if (h > 0) {
        const float d = f[-sh] - f[0];
        g = g - (double)d / sqrt((double)d * (double)d + 1e-6);
    }
    if (w + 1 < W) {
        const float d = f[0] - f[sw];
        g = g + (double)d / sqrt((double)d * (double)d + 1e-6);
    }
    if (w > 0) {
        const float d = f[-sw] - f[0];
        g = g - (double)d / sqrt((double)d * (double)d + 1e-6);
    }
    return g;
}

// one thread per source pixel key; grad_flow [B, 2, H, W] contiguous, every element written once
__global__ void warping_backward(BwdArgs a, const uint32_t *__restrict__ perm, const uint32_t *__restrict__ seg, double weight,
                                 const float *__restrict__ grad_out, float *__restrict__ grad_flow) {
    const int64_t key = (int64_t)blockIdx.x * kBlock + threadIdx.x, P = (int64_t)a.H * a.W;
    const bool valid = key < a.B * P;
    uint32_t s = 0, e = 0;
    float fy = 0.f, fx = 0.f;
    const float *f = a.flow.p;
    int h = 0, w = 0;
    if (valid) {
        s = seg[key], e = seg[key + 1];
        const int64_t b = key / P, pix = key % P;
        h = (int)(pix / a.W), w = (int)(pix % a.W);
        f = a.flow.p + b * a.flow.sb + h * a.flow.sh + w * a.flow.sw;
        fx = f[0];
        fy = f[a.flow.sc];
    }
    double gy = 0.0, gx = 0.0;
    const bool is_long = e - s >= kLongRun;
    if (!is_long) {
        for (uint32_t j = s; j < e; ++j) {
            double ey, ex;
            event_gradient(a, perm[j], fy, fx, &ey, &ex);
            gy = gy + ey;
            gx = gx + ex;
        }
    }
    const int lane = threadIdx.x & 63;
    unsigned long long todo = __ballot(is_long);
    while (todo) {
        const int owner = __ffsll((long long)todo) - 1;
        todo &= todo - 1;
        const uint32_t ls = (uint32_t)__shfl((int)s, owner), le = (uint32_t)__shfl((int)e, owner);
        const float ofy = __shfl(fy, owner), ofx = __shfl(fx, owner);
        double ry = 0.0, rx = 0.0;
        for (uint32_t j = ls; j < le; j += 64) {
            const uint32_t cnt = le - j < 64u ? le - j : 64u;
            double ey = 0.0, ex = 0.0;
            if ((uint32_t)lane < cnt) event_gradient(a, perm[j + lane], ofy, ofx, &ey, &ex);
            for (uint32_t k = 0; k < cnt; ++k) {      // lane order == event order
                ry = ry + __shfl(ey, (int)k);
                rx = rx + __shfl(ex, (int)k);
            }
        }
        if (lane == owner) gy = ry, gx = rx;
    }
    if (!valid) return;
    const double g = (double)grad_out[0];
    const double smx = smooth_gradient(f, h, w, a.H, a.W, a.flow.sh, a.flow.sw);
    const double smy = smooth_gradient(f + a.flow.sc, h, w, a.H, a.W, a.flow.sh, a.flow.sw);
    const int64_t b = key / P, pix = key % P;
    grad_flow[(b * 2) * P + pix] = (float)(g * (gx + weight * smx));
    grad_flow[(b * 2 + 1) * P + pix] = (float)(g * (gy + weight * smy));
}

// ------------------------------------------------------------------ AveragedIWE
// perm: the events sorted by (destination, source, polarity class), stable.  One thread per destination key counts, per
// polarity, the (source, polarity) groups of its run -- the number of distinct source pixels -- and divides the count image.
__global__ void averaged_divide(const uint32_t *__restrict__ perm, const uint32_t *__restrict__ seg,
                                const uint32_t *__restrict__ src_keys, const uint32_t *__restrict__ pol_keys, int64_t nkeys,
                                int64_t P, float *__restrict__ out /* [B, 2, P]: the counts, divided in place */) {
    const int64_t key = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const bool valid = key < nkeys;
    uint32_t s = 0, e = 0;
    if (valid) s = seg[key], e = seg[key + 1];
    uint32_t cnt[2] = {0u, 0u};
    const bool is_long = e - s >= kLongRun;
    if (!is_long) {
        uint32_t ps = 0, pp = 0;
        for (uint32_t j = s; j < e; ++j) {
            const uint32_t g = perm[j], sk = src_keys[g], pk = pol_keys[g];
            if ((j == s || sk != ps || pk != pp) && pk < 2u) cnt[pk] += 1u;
            ps = sk, pp = pk;
        }
    }
    const int lane = threadIdx.x & 63;
    unsigned long long todo = __ballot(is_long);
    while (todo) {
        const int owner = __ffsll((long long)todo) - 1;
        todo &= todo - 1;
        const uint32_t ls = (uint32_t)__shfl((int)s, owner), le = (uint32_t)__shfl((int)e, owner);
        uint32_t c0 = 0, c1 = 0;
        for (uint32_t j = ls + lane; j < le; j += 64) {
            const uint32_t g = perm[j], sk = src_keys[g], pk = pol_keys[g];
            bool first = j == ls;
            if (!first) {
                const uint32_t g0 = perm[j - 1];
                first = src_keys[g0] != sk || pol_keys[g0] != pk;
            }
            if (first && pk == 0u) c0 += 1u;
            if (first && pk == 1u) c1 += 1u;
        }
        for (int d = 32; d > 0; d >>= 1) {      // integers: any order gives the same sum
            c0 += (uint32_t)__shfl_xor((int)c0, d);
            c1 += (uint32_t)__shfl_xor((int)c1, d);
        }
        if (lane == owner) cnt[0] = c0, cnt[1] = c1;
    }
    if (!valid) return;
    const int64_t b = key / P, pix = key % P;
    // channel 0 = positive (polarity class 1), channel 1 = negative (class 0)
    float *pos = out + (b * 2) * P + pix, *neg = out + (b * 2 + 1) * P + pix;
    if (cnt[1] > 0u) *pos = *pos / (float)cnt[1];
    if (cnt[0] > 0u) *neg = *neg / (float)cnt[0];
}

// ------------------------------------------------------------------ host side
constexpr size_t kAlign = 256;
inline size_t up(size_t v) { return (v + kAlign - 1) / kAlign * kAlign; }

constexpr int64_t kMaxEntries = ((int64_t)1 << 32) - 1;      // 4 * B * N: permutation entries and table sums are uint32
constexpr int64_t kMaxKeys = ((int64_t)1 << 32) - 2;         // B * H * W: the unread key B * H * W must fit

struct Sort {
    uint32_t *keys[2], *perm[2], *hist, *sums;
    int64_t nb, m, nt;
};

struct Layout {
    size_t keys[2], perm[2], hist, sums, seg;          // the destination sort over up to 4 B N entries
    size_t keys2[2], perm2[2], seg2;                   // the second index (AveragedIWE), B N entries
    size_t idx, w, src, pol, partials, total;
    int64_t nb, m, nt, npart;
};

Layout layout(int64_t B, int64_t N, int64_t P) {
    Layout L;
    const int64_t n = 4 * B * N, ne = B * N, K = B * P;
    L.nb = ceil_div(n, kBlock);
    L.m = 256 * L.nb;
    L.nt = ceil_div(L.m, kScanTile);
    L.npart = ceil_div(4 * K, kBlock);
    size_t at = 0;
    auto take = [&at](size_t bytes) {
        const size_t here = at;
        at += up(bytes);
        return here;
    };
    for (int k = 0; k < 2; ++k) L.keys[k] = take((size_t)n * 4);
    for (int k = 0; k < 2; ++k) L.perm[k] = take((size_t)n * 4);
    L.hist = take((size_t)L.m * 4);
    L.sums = take((size_t)L.nt * 4);
    L.seg = take((size_t)(K + 2) * 4);
    for (int k = 0; k < 2; ++k) L.keys2[k] = take((size_t)ne * 4);
    for (int k = 0; k < 2; ++k) L.perm2[k] = take((size_t)ne * 4);
    L.seg2 = take((size_t)(K + 2) * 4);
    L.idx = take((size_t)n * 4);
    L.w = take((size_t)n * 4);
    L.src = take((size_t)ne * 4);
    L.pol = take((size_t)ne * 4);
    L.partials = take((size_t)L.npart * 8);
    L.total = at;
    return L;
}

// the source-pixel index of the gradient: its own, smaller buffer (B N entries), kept by the caller between the two calls
struct IndexLayout {
    size_t keys[2], perm[2], hist, sums, seg, total;
};

IndexLayout index_layout(int64_t B, int64_t N, int64_t P) {
    IndexLayout L;
    const int64_t ne = B * N, m = 256 * ceil_div(ne, kBlock);
    size_t at = 0;
    auto take = [&at](size_t bytes) {
        const size_t here = at;
        at += up(bytes);
        return here;
    };
    for (int k = 0; k < 2; ++k) L.perm[k] = take((size_t)ne * 4);
    L.seg = take((size_t)(B * P + 2) * 4);
    for (int k = 0; k < 2; ++k) L.keys[k] = take((size_t)ne * 4);
    L.hist = take((size_t)m * 4);
    L.sums = take((size_t)ceil_div(m, kScanTile) * 4);
    L.total = at;
    return L;
}

template <typename T>
T *at(void *ws, size_t off) {
    return reinterpret_cast<T *>(static_cast<char *>(ws) + off);
}

Sort sort_main(void *ws, const Layout &L) {
    Sort S;
    for (int k = 0; k < 2; ++k) S.keys[k] = at<uint32_t>(ws, L.keys[k]), S.perm[k] = at<uint32_t>(ws, L.perm[k]);
    S.hist = at<uint32_t>(ws, L.hist), S.sums = at<uint32_t>(ws, L.sums);
    return S;
}

Sort sort_second(void *ws, const Layout &L) {
    Sort S = sort_main(ws, L);
    for (int k = 0; k < 2; ++k) S.keys[k] = at<uint32_t>(ws, L.keys2[k]), S.perm[k] = at<uint32_t>(ws, L.perm2[k]);
    return S;
}

#define IWE_LAUNCH(label, kern, grid, ...)                                                \
    {                                                                                     \
        {                                                                                 \
            ProfScope ps_(label, st);                                                     \
            hipLaunchKernelGGL(kern, grid, dim3(kBlock), 0, st, __VA_ARGS__);             \
        }                                                                                 \
        if (int rc = check_launch(label)) return rc;                                      \
    }

int key_passes(int64_t maxkey) {
    int bits = 0;
    while (bits < 32 && ((uint64_t)maxkey >> bits) != 0) ++bits;
    return bits == 0 ? 1 : (bits + 7) / 8;
}

// Sorts n entries (n >= 1) whose keys lie in [0, maxkey] and stand in S.keys[*cur]; with_perm: S.perm[*cur] holds the
// permutation so far (a more significant key over an earlier sort), else it is the identity.  *cur names the result.
int radix_sort(Sort &S, int64_t n, int64_t maxkey, bool with_perm, int *cur, hipStream_t st) {
    S.nb = ceil_div(n, kBlock);
    S.m = 256 * S.nb;
    S.nt = ceil_div(S.m, kScanTile);
    const int passes = key_passes(maxkey);
    for (int p = 0; p < passes; ++p) {
        const int shift = 8 * p, c = *cur;
        IWE_LAUNCH("iwe_sort_hist", sort_hist, dim3((unsigned)S.nb), S.keys[c], n, shift, S.hist, (int)S.nb);
        IWE_LAUNCH("iwe_scan_tiles", scan_tiles, dim3((unsigned)S.nt), S.hist, S.m, S.sums);
        IWE_LAUNCH("iwe_scan_sums", scan_sums, dim3(1), S.sums, S.nt);
        IWE_LAUNCH("iwe_sort_scatter", sort_scatter, dim3((unsigned)S.nb), S.keys[c],
                   (p == 0 && !with_perm) ? (const uint32_t *)nullptr : S.perm[c], n, shift, S.hist, S.sums, (int)S.nb,
                   S.keys[c ^ 1], S.perm[c ^ 1]);
        *cur = c ^ 1;
    }
    return EBFI_OK;
}

int starts(const uint32_t *keys, int64_t n, int64_t nkeys, uint32_t *seg, hipStream_t st) {
    IWE_LAUNCH("iwe_run_starts", run_starts, dim3((unsigned)ceil_div(nkeys + 1, kBlock)), keys, n, nkeys, seg);
    return EBFI_OK;
}

int sizes_ok(const char *what, int64_t B, int64_t N, int H, int W) {
    if (B < 1 || N < 0 || H < 1 || W < 1) return fail(EBFI_ERR_ARG, "%s: bad sizes", what);
    if (N > kMaxEntries / 4 / B || (int64_t)H * W > kMaxKeys / B)
        return fail(EBFI_ERR_UNSUPPORTED, "%s: 4 * B * N >= 2^32 or B * H * W >= 2^32 - 1", what);
    return EBFI_OK;
}

int workspace_ok(const char *what, int64_t B, int64_t N, int H, int W, const void *ws, int64_t bytes) {
    if (!ws || bytes < (int64_t)layout(B, N, (int64_t)H * W).total) return fail(EBFI_ERR_WORKSPACE, "%s: workspace too small", what);
    if (!aligned16(ws)) return fail(EBFI_ERR_ARG, "%s: workspace not 16-byte aligned", what);
    return EBFI_OK;
}

int index_ok(const char *what, int64_t B, int64_t N, int H, int W, const void *index, int64_t bytes) {
    if (!index || bytes < (int64_t)index_layout(B, N, (int64_t)H * W).total) return fail(EBFI_ERR_WORKSPACE, "%s: index too small", what);
    if (!aligned16(index)) return fail(EBFI_ERR_ARG, "%s: index not 16-byte aligned", what);
    return EBFI_OK;
}

// keys in S.keys[0] (n entries) -> sorted, run starts in seg, then the ordered accumulation into out [B, planes, P]
int sort_and_accumulate(Sort &S, uint32_t *seg, const AccArgs &a, int64_t n, int64_t B, int64_t P, int planes, float *out,
                        hipStream_t st) {
    int cur = 0;
    if (int rc = radix_sort(S, n, B * P, false, &cur, st)) return rc;
    if (int rc = starts(S.keys[cur], n, B * P, seg, st)) return rc;
    const dim3 grid((unsigned)ceil_div(B * P, kBlock));
    if (planes == 1) {
        IWE_LAUNCH("iwe_accumulate", accumulate<1>, grid, a, S.perm[cur], seg, B * P, P, out);
    } else if (planes == 2) {
        IWE_LAUNCH("iwe_accumulate", accumulate<2>, grid, a, S.perm[cur], seg, B * P, P, out);
    } else {
        IWE_LAUNCH("iwe_accumulate", accumulate<4>, grid, a, S.perm[cur], seg, B * P, P, out);
    }
    return EBFI_OK;
}

int zero(void *p, size_t bytes, hipStream_t st, const char *what) {
    if (bytes && hipMemsetAsync(p, 0, bytes, st) != hipSuccess) return fail(EBFI_ERR_LAUNCH, "%s: memset failed", what);
    return EBFI_OK;
}

}  // namespace

extern "C" int64_t ebfi_iwe_workspace(int64_t B, int64_t N, int H, int W) {
    if (B < 1 || N < 0 || H < 1 || W < 1 || N > kMaxEntries / 4 / B || (int64_t)H * W > kMaxKeys / B) return 0;
    return (int64_t)layout(B, N, (int64_t)H * W).total;
}

extern "C" int64_t ebfi_iwe_index_bytes(int64_t B, int64_t N, int H, int W) {
    if (ebfi_iwe_workspace(B, N, H, W) == 0) return 0;
    return (int64_t)index_layout(B, N, (int64_t)H * W).total;
}

extern "C" int ebfi_iwe_get_interpolation(const float *events, const float *flow_ev, int64_t B, int64_t N, float tref, int H, int W,
                                          float flow_scaling, int round_idx, float *idx, float *weights, void *stream) {
    if (int rc = sizes_ok("iwe_get_interpolation", B, N, H, W)) return rc;
    if (N == 0) return EBFI_OK;
    if (!events || !flow_ev || !idx || !weights) return fail(EBFI_ERR_ARG, "iwe_get_interpolation: null pointer");
    hipStream_t st = static_cast<hipStream_t>(stream);
    IWE_LAUNCH("iwe_warp_events", warp_events, dim3((unsigned)ceil_div(B * N, kBlock)), events, flow_ev, Flow4{nullptr, 0, 0, 0, 0}, B,
               N, tref, flow_scaling, round_idx ? 1 : 0, H, W, idx, weights, (uint32_t *)nullptr, (uint32_t *)nullptr,
               (uint32_t *)nullptr);
    return EBFI_OK;
}

extern "C" int ebfi_iwe_interpolate(const void *idx, int idx_is_i64, const float *weights, const float *polarity_mask, int64_t B,
                                    int64_t M, int H, int W, float *out, void *workspace, int64_t workspace_bytes, void *stream) {
    const int64_t N4 = M < 0 ? -1 : (M + 3) / 4;
    if (int rc = sizes_ok("iwe_interpolate", B, N4, H, W)) return rc;
    if (!out) return fail(EBFI_ERR_ARG, "iwe_interpolate: null output");
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int64_t P = (int64_t)H * W;
    if (M == 0) return zero(out, (size_t)(B * P) * 4, st, "iwe_interpolate");
    if (!idx || !weights) return fail(EBFI_ERR_ARG, "iwe_interpolate: null pointer");
    if (int rc = workspace_ok("iwe_interpolate", B, N4, H, W, workspace, workspace_bytes)) return rc;
    const Layout L = layout(B, N4, P);
    Sort S = sort_main(workspace, L);
    IWE_LAUNCH("iwe_interpolate_keys", interpolate_keys, dim3((unsigned)ceil_div(B * M, kBlock)), idx, idx_is_i64 ? 1 : 0, B, M, P,
               S.keys[0]);
    const AccArgs a{weights, polarity_mask, nullptr, nullptr, 1, M, M, 0};
    return sort_and_accumulate(S, at<uint32_t>(workspace, L.seg), a, B * M, B, P, 1, out, st);
}

extern "C" int ebfi_iwe_deblur(const float *flow, int64_t flow_sb, int64_t flow_sc, int64_t flow_sh, int64_t flow_sw,
                               const float *events, int64_t B, int64_t N, int H, int W, float flow_scaling, int round_idx,
                               int planes, const float *mask_a, const float *mask_b, int64_t mask_stride, float *out,
                               void *workspace, int64_t workspace_bytes, void *stream) {
    if (int rc = sizes_ok("iwe_deblur", B, N, H, W)) return rc;
    if (planes != 1 && planes != 2) return fail(EBFI_ERR_ARG, "iwe_deblur: planes must be 1 or 2, got %d", planes);
    if (!out) return fail(EBFI_ERR_ARG, "iwe_deblur: null output");
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int64_t P = (int64_t)H * W;
    if (N == 0) return zero(out, (size_t)(B * planes * P) * 4, st, "iwe_deblur");      // (an empty list has null masks)
    if (!flow || !events) return fail(EBFI_ERR_ARG, "iwe_deblur: null pointer");
    if (planes == 2 && (!mask_a || !mask_b)) return fail(EBFI_ERR_ARG, "iwe_deblur: two planes need two masks");
    if (planes == 1) mask_b = nullptr;
    if (int rc = workspace_ok("iwe_deblur", B, N, H, W, workspace, workspace_bytes)) return rc;
    const Layout L = layout(B, N, P);
    Sort S = sort_main(workspace, L);
    float *w = at<float>(workspace, L.w);
    const int64_t M = (round_idx ? 1 : 4) * N;
    IWE_LAUNCH("iwe_warp_events", warp_events, dim3((unsigned)ceil_div(B * N, kBlock)), events, (const float *)nullptr,
               Flow4{flow, flow_sb, flow_sc, flow_sh, flow_sw}, B, N, 1.f, flow_scaling, round_idx ? 1 : 0, H, W, (float *)nullptr, w,
               S.keys[0], (uint32_t *)nullptr, (uint32_t *)nullptr);
    const AccArgs a{w, mask_a, mask_b, events, mask_stride, N, M, 0};
    return sort_and_accumulate(S, at<uint32_t>(workspace, L.seg), a, B * M, B, P, planes, out, st);
}

extern "C" int ebfi_iwe_source_index(const float *events, int64_t B, int64_t N, int H, int W, void *index, int64_t index_bytes,
                                     void *stream) {
    if (int rc = sizes_ok("iwe_source_index", B, N, H, W)) return rc;
    if (int rc = index_ok("iwe_source_index", B, N, H, W, index, index_bytes)) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int64_t P = (int64_t)H * W;
    const IndexLayout L = index_layout(B, N, P);
    uint32_t *seg = at<uint32_t>(index, L.seg);
    if (N == 0) return zero(seg, (size_t)(B * P + 2) * 4, st, "iwe_source_index");
    if (!events) return fail(EBFI_ERR_ARG, "iwe_source_index: null pointer");
    Sort S;
    for (int k = 0; k < 2; ++k) S.keys[k] = at<uint32_t>(index, L.keys[k]), S.perm[k] = at<uint32_t>(index, L.perm[k]);
    S.hist = at<uint32_t>(index, L.hist), S.sums = at<uint32_t>(index, L.sums);
    IWE_LAUNCH("iwe_source_keys", source_keys, dim3((unsigned)ceil_div(B * N, kBlock)), events, B, N, H, W, S.keys[0]);
    int cur = 0;
    if (int rc = radix_sort(S, B * N, B * P, false, &cur, st)) return rc;
    return starts(S.keys[cur], B * N, B * P, seg, st);
}

extern "C" int ebfi_iwe_warping_forward(const float *flow, int64_t flow_sb, int64_t flow_sc, int64_t flow_sh, int64_t flow_sw,
                                        const float *events, const float *pol_mask, int64_t B, int64_t N, int H, int W,
                                        float flow_scaling, double weight, float *images, float *loss, void *workspace,
                                        int64_t workspace_bytes, void *stream) {
    if (int rc = sizes_ok("iwe_warping_forward", B, N, H, W)) return rc;
    if (!flow || !images || !loss || (N > 0 && (!events || !pol_mask))) return fail(EBFI_ERR_ARG, "iwe_warping_forward: null pointer");
    if (int rc = workspace_ok("iwe_warping_forward", B, N, H, W, workspace, workspace_bytes)) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int64_t P = (int64_t)H * W;
    const Layout L = layout(B, N, P);
    const Flow4 F{flow, flow_sb, flow_sc, flow_sh, flow_sw};
    if (N == 0) {
        if (int rc = zero(images, (size_t)(8 * B * P) * 4, st, "iwe_warping_forward")) return rc;
    } else {
        Sort S = sort_main(workspace, L);
        float *w = at<float>(workspace, L.w);
        for (int d = 0; d < 2; ++d) {      // tref = 1 with stamp weights ts, then tref = 0 with 1 - ts; one sort each
            IWE_LAUNCH("iwe_warp_events", warp_events, dim3((unsigned)ceil_div(B * N, kBlock)), events, (const float *)nullptr, F, B,
                       N, d == 0 ? 1.f : 0.f, flow_scaling, 0, H, W, (float *)nullptr, w, S.keys[0], (uint32_t *)nullptr,
                       (uint32_t *)nullptr);
            const AccArgs a{w, pol_mask, pol_mask + 1, events, 2, N, 4 * N, d == 0 ? 1 : 2};
            if (int rc = sort_and_accumulate(S, at<uint32_t>(workspace, L.seg), a, 4 * B * N, B, P, 4, images + (int64_t)d * B * 4 * P, st))
                return rc;
        }
    }
    double *partials = at<double>(workspace, L.partials);
    IWE_LAUNCH("iwe_loss_partials", loss_partials, dim3((unsigned)L.npart), images, F, B, H, W, weight, partials);
    IWE_LAUNCH("iwe_loss_final", loss_final, dim3(1), partials, L.npart, loss);
    return EBFI_OK;
}

extern "C" int ebfi_iwe_warping_backward(const float *flow, int64_t flow_sb, int64_t flow_sc, int64_t flow_sh, int64_t flow_sw,
                                         const float *events, const float *pol_mask, int64_t B, int64_t N, int H, int W,
                                         float flow_scaling, double weight, const float *images, const void *index,
                                         int64_t index_bytes, const float *grad_out, float *grad_flow, void *stream) {
    if (int rc = sizes_ok("iwe_warping_backward", B, N, H, W)) return rc;
    if (!flow || !images || !grad_out || !grad_flow || (N > 0 && (!events || !pol_mask)))
        return fail(EBFI_ERR_ARG, "iwe_warping_backward: null pointer");
    if (int rc = index_ok("iwe_warping_backward", B, N, H, W, index, index_bytes)) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int64_t P = (int64_t)H * W;
    const IndexLayout L = index_layout(B, N, P);
    // the index as ebfi_iwe_source_index left it: the sorted permutation stands where the last pass wrote it
    const int cur = N == 0 ? 0 : key_passes(B * P) & 1;
    const uint32_t *perm = at<const uint32_t>(const_cast<void *>(index), L.perm[cur]);
    const uint32_t *seg = at<const uint32_t>(const_cast<void *>(index), L.seg);
    const BwdArgs a{events, pol_mask, images, Flow4{flow, flow_sb, flow_sc, flow_sh, flow_sw}, B, N, H, W, flow_scaling};
    IWE_LAUNCH("iwe_warping_backward", warping_backward, dim3((unsigned)ceil_div(B * P, kBlock)), a, perm, seg, weight, grad_out,
               grad_flow);
    return EBFI_OK;
}

extern "C" int ebfi_iwe_averaged(const float *flow, int64_t flow_sb, int64_t flow_sc, int64_t flow_sh, int64_t flow_sw,
                                 const float *events, const float *pol_mask, int64_t B, int64_t N, int H, int W, float flow_scaling,
                                 float *out, void *workspace, int64_t workspace_bytes, void *stream) {
    if (int rc = sizes_ok("iwe_averaged", B, N, H, W)) return rc;
    if (!out) return fail(EBFI_ERR_ARG, "iwe_averaged: null output");
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int64_t P = (int64_t)H * W;
    if (N == 0) return zero(out, (size_t)(2 * B * P) * 4, st, "iwe_averaged");
    if (!flow || !events || !pol_mask) return fail(EBFI_ERR_ARG, "iwe_averaged: null pointer");
    if (int rc = workspace_ok("iwe_averaged", B, N, H, W, workspace, workspace_bytes)) return rc;
    const Layout L = layout(B, N, P);
    Sort S = sort_main(workspace, L);
    float *w = at<float>(workspace, L.w);
    uint32_t *src = at<uint32_t>(workspace, L.src), *pol = at<uint32_t>(workspace, L.pol);
    // the destination keys stay in idx's place for the second index (the first sort consumes its own copy)
    uint32_t *dst = at<uint32_t>(workspace, L.idx);
    IWE_LAUNCH("iwe_warp_events", warp_events, dim3((unsigned)ceil_div(B * N, kBlock)), events, (const float *)nullptr,
               Flow4{flow, flow_sb, flow_sc, flow_sh, flow_sw}, B, N, 1.f, flow_scaling, 1, H, W, (float *)nullptr, w, dst, src, pol);
    const int64_t n = B * N;
    // 1. the per-polarity counts, by the ordered scatter
    IWE_LAUNCH("iwe_gather_keys", gather_keys, dim3((unsigned)ceil_div(n, kBlock)), dst, (const uint32_t *)nullptr, n, S.keys[0]);
    const AccArgs a{w, pol_mask, pol_mask + 1, events, 2, N, N, 0};
    if (int rc = sort_and_accumulate(S, at<uint32_t>(workspace, L.seg), a, n, B, P, 2, out, st)) return rc;
    // 2. three stable sorts, least significant key first: polarity class, source pixel, destination pixel
    Sort T = sort_second(workspace, L);
    int cur = 0;
    IWE_LAUNCH("iwe_gather_keys", gather_keys, dim3((unsigned)ceil_div(n, kBlock)), pol, (const uint32_t *)nullptr, n, T.keys[0]);
    if (int rc = radix_sort(T, n, 2, false, &cur, st)) return rc;
    IWE_LAUNCH("iwe_gather_keys", gather_keys, dim3((unsigned)ceil_div(n, kBlock)), src, T.perm[cur], n, T.keys[cur]);
    if (int rc = radix_sort(T, n, B * P, true, &cur, st)) return rc;
    IWE_LAUNCH("iwe_gather_keys", gather_keys, dim3((unsigned)ceil_div(n, kBlock)), dst, T.perm[cur], n, T.keys[cur]);
    if (int rc = radix_sort(T, n, B * P, true, &cur, st)) return rc;
    uint32_t *seg2 = at<uint32_t>(workspace, L.seg2);
    if (int rc = starts(T.keys[cur], n, B * P, seg2, st)) return rc;
    IWE_LAUNCH("iwe_averaged_divide", averaged_divide, dim3((unsigned)ceil_div(B * P, kBlock)), T.perm[cur], seg2, src, pol, B * P, P,
               out);
    return EBFI_OK;
}
