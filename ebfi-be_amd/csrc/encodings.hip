// The rest of dataloader/encodings.py on the device: event list -> images, voxel grids, stacks, channels and masks
// (reference: encodings.py:8-74 image / bilinear image, :102-150 voxel grid, :204-240 stack without polarity, :243-268 image,
// :271-286 voxel from normalised stamps, :289-304 channels, :353-377 mask, :380-391 polarity mask, :394-409 hot-pixel mask,
// :412-430 stack2cnt).
//
// THE LAW.  Every one of those functions is an index_put_(accumulate=True) of fractional fp32 weights, and with one thread (or
// under torch.use_deterministic_algorithms) that is a serial sum: each pixel receives its addends in EVENT-LIST ORDER, every
// product and sum rounded to fp32, nothing fused.  Float atomics cannot give that (their order is the arrival order), so the
// scatter is turned into a gather:
//   1. grid_keys      one thread per event: the destination pixel key (out-of-range events -> pixel (0,0), as the reference's
//                     in-place zeroing of xs / ys does)
//   2. a STABLE least-significant-digit radix sort of (key, event index) on 8-bit digits: per pass a 256-bin histogram per
//      workgroup of 256 events (integer LDS atomics), an exclusive scan over the [digit][workgroup] table, and a scatter whose
//      rank inside the workgroup is (events of the same digit in earlier waves) + (earlier lanes of the same digit in this wave:
//      eight ballots).  Integer arithmetic only: the permutation is a function of the keys, not of timing, and a pixel that owns
//      every event costs exactly what a uniform list costs.
//   3. grid_segments  one thread per pixel: the start of its run in the sorted keys (bisection)
//   4. the accumulation: one thread per (pixel, plane) walks the pixel's run -- ascending event index, because the sort is
//      stable -- and adds in that order; a run of 64 events or more is gathered by the whole wave, 64 events at a time, and
//      summed over the lanes in lane order: the same adds in the same order.  No output element is touched by two threads;
//      nothing is zeroed first.
// The index depends on the coordinates only; one call builds it once and all planes use it.  Nothing is read back: `n <= 3` is
// decided from n, "all stamps zero" on the device (sorted non-negative stamps: first == last == 0, as events_bounds does).
// All launches go onto `stream`, one after the other: capturable, a single chain.
//
// The reference's in-place side effects are reproduced in closed form per mode (the caller's arrays are never written): see
// include/ebfi_hip.h and DESIGN.md.
#include "common.hpp"

// Every product and sum below is its own rounding: contraction is off for this file, and the arithmetic is written with plain
// operators, which the pragma governs (the __f*_rn helpers are inline `x * y` in a header the pragma does not reach, and their
// results were seen fused into the following add).
#pragma clang fp contract(off)

using namespace ebfi;

namespace {

constexpr int kBlock = 256;        // events per sort workgroup, pixels per accumulation workgroup
constexpr int kScanTile = 1024;    // table entries per scan workgroup (4 per thread)

// coordinates that the reference keeps (everything else it moves to pixel (0,0) with weight 0); a NaN counts as out of range
__device__ __forceinline__ bool in_range(float x, float y, int H, int W) {
    return x >= 0.f && x < (float)W && y >= 0.f && y < (float)H;
}

// ------------------------------------------------------------------ keys
__global__ void grid_keys(const float *__restrict__ xs, const float *__restrict__ ys, int64_t n, int H, int W,
                          uint32_t *__restrict__ keys) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const float x = xs[i], y = ys[i];
    keys[i] = in_range(x, y, H, W) ? (uint32_t)((int)y * W + (int)x) : 0u;      // .long(): truncation
}

// events_to_image_torch(interpolation='bilinear'): the per-event base pixel, fractions and masked weight, as
// encodings.py:36-41, :50-66 form them (pad = 1: image [H+1, W+1], the clip mask never fires; pad = 0: clip_out_of_range)
__global__ void bilinear_prepare(const float *__restrict__ xs, const float *__restrict__ ys, const float *__restrict__ ps,
                                 int64_t n, int H, int W, int pad, int64_t *__restrict__ pxs, int64_t *__restrict__ pys,
                                 float *__restrict__ dxs, float *__restrict__ dys, float *__restrict__ ws) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    float x = xs[i], y = ys[i], p = ps[i];
    if (!in_range(x, y, H, W)) x = 0.f, y = 0.f, p = 0.f;
    const float clipx = (float)(W + pad - 1), clipy = (float)(H + pad - 1);
    const float mask = (x >= clipx ? 0.f : 1.f) * (y >= clipy ? 0.f : 1.f);
    const float fx = floorf(x), fy = floorf(y);
    dxs[i] = x - fx;
    dys[i] = y - fy;
    pxs[i] = (int64_t)(fx * mask);
    pys[i] = (int64_t)(fy * mask);
    ws[i] = p * mask;
}

// interpolate_to_image: key of the base pixel; an event whose 2 x 2 footprint leaves the image goes to the unread key H * W
__global__ void bilinear_keys(const int64_t *__restrict__ pxs, const int64_t *__restrict__ pys, int64_t n, int H, int W,
                              uint32_t *__restrict__ keys) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const int64_t x = pxs[i], y = pys[i];
    const bool ok = x >= 0 && x <= (int64_t)W - 2 && y >= 0 && y <= (int64_t)H - 2;
    keys[i] = ok ? (uint32_t)(y * W + x) : (uint32_t)H * (uint32_t)W;
}

// ------------------------------------------------------------------ stable LSD radix sort, 8 bits per pass
// hist[d * nb + b]: events of digit d in workgroup b -- the order in which a stable scatter consumes output slots
__global__ void sort_hist(const uint32_t *__restrict__ keys, int64_t n, int shift, uint32_t *__restrict__ hist, int nb) {
    __shared__ uint32_t h[256];
    h[threadIdx.x] = 0;
    __syncthreads();
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i < n) atomicAdd(&h[(keys[i] >> shift) & 255u], 1u);
    __syncthreads();
    hist[(int64_t)threadIdx.x * nb + blockIdx.x] = h[threadIdx.x];
}

// exclusive scan of 256 values, one per thread (Hillis-Steele in LDS); returns the value's prefix, *total the sum
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

// table[m] -> exclusive scan inside every tile of 1024 entries (in place), sums[tile] = the tile's total
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

// sums[nt] -> exclusive scan in place, one workgroup, 256 entries per round with a running carry
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

// perm_in == nullptr: the first pass, the permutation is the identity
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
    // lanes of this wave that hold the same digit
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
    keys_out[at] = key;                  // at < n: the table counts exactly the n active events
    perm_out[at] = perm_in ? perm_in[i] : (uint32_t)i;
}

// seg[k] = first position of the sorted keys that is >= k, for k in [0, nkeys]
__global__ void grid_segments(const uint32_t *__restrict__ keys, int64_t n, int64_t nkeys, uint32_t *__restrict__ seg) {
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

// ------------------------------------------------------------------ time bins of the naive modes (fp32, as the reference)
__device__ int64_t ref_bsearch32(const float *__restrict__ t, int64_t l, int64_t r, float x, bool left) {
    while (l <= r) {
        if (t[l] == x) return l;
        if (t[r] == x) return r;
        const int64_t mid = l + (r - l) / 2;
        const float mv = t[mid];
        if (mv == x) return mid;
        else if (mv < x) l = mid + 1;
        else r = mid - 1;
    }
    return left ? l : r;
}

// bounds[2b] = beg, bounds[2b+1] = end of bin b (encodings.py:129-144, :224-230); all 0 when the result must stay zero
__global__ void grid_bounds(const float *__restrict__ ts, int64_t n, int bins, int64_t *__restrict__ bounds) {
    const int bi = blockIdx.x * blockDim.x + threadIdx.x;
    if (bi >= bins) return;
    const bool empty = (n <= 3) || (ts[0] == 0.f && ts[n - 1] == 0.f);
    if (empty) {
        bounds[2 * bi] = 0;
        bounds[2 * bi + 1] = 0;
        return;
    }
    const float dt = (ts[n - 1] - ts[0]) + 1e-6f;
    const float delta_t = dt / (float)bins;
    const float tstart = ts[0] + delta_t * (float)bi;
    const float tend = tstart + delta_t;
    bounds[2 * bi] = ref_bsearch32(ts, 0, n - 1, tstart, true);
    bounds[2 * bi + 1] = ref_bsearch32(ts, 0, n - 1, tend, false) + 1;
}

// ------------------------------------------------------------------ accumulation: one thread per (pixel, plane)
// what the modes need per plane, the same for every lane of a launch row
struct PlaneCtx {
    int b, H, W;
    int64_t beg, end;        // naive modes: the plane's slice of the event list
    float t0, dt, scale, fb; // voxel modes
    bool empty;              // voxel_torch: all stamps zero
};

// the addend of event i in plane c.b; false: the event does not take part (an add that the reference does not make)
template <int MODE>
__device__ __forceinline__ bool grid_addend(uint32_t i, const PlaneCtx &c, const float *__restrict__ xs,
                                            const float *__restrict__ ys, const float *__restrict__ ts,
                                            const float *__restrict__ ps, float *a) {
    if (MODE == EBFI_GRID_IMAGE) {
        *a = in_range(xs[i], ys[i], c.H, c.W) ? ps[i] : 0.f;
        return true;
    } else if (MODE == EBFI_GRID_CHANNELS) {
        const float p = ps[i];
        if (c.b == 0) {        // the positive pass zeroes the weight of an out-of-range event ...
            const float w = p * (p < 0.f ? 0.f : p);
            *a = in_range(xs[i], ys[i], c.H, c.W) ? w : 0.f;
        } else {               // ... and moves it: the negative pass finds it at (0,0) with its weight intact
            *a = p * (p > 0.f ? 0.f : p);
        }
        return true;
    } else if (MODE == EBFI_GRID_VOXEL_BILINEAR || MODE == EBFI_GRID_VOXEL_NORMALISED) {
        if (c.empty) return false;
        const float t = ts[i];
        const float tn = MODE == EBFI_GRID_VOXEL_BILINEAR ? (t - c.t0) / c.dt * c.scale : t * c.scale;
        const float w = fmaxf(0.f, 1.f - fabsf(tn - c.fb));
        const float v = ps[i] * w;
        // bin 0 zeroes the weight of an out-of-range event and moves it to (0,0); every later bin counts it there
        *a = (c.b == 0 && !in_range(xs[i], ys[i], c.H, c.W)) ? 0.f : v;
        return true;
    } else {   // EBFI_GRID_VOXEL_NAIVE, EBFI_GRID_STACK_NO_POLARITY: ps[beg:end] itself is zeroed, so such an event adds 0 for good
        if ((int64_t)i < c.beg || (int64_t)i >= c.end) return false;
        *a = in_range(xs[i], ys[i], c.H, c.W) ? ps[i] : 0.f;
        return true;
    }
}

// Runs shorter than kLongRun are walked by their own lane.  A longer run (a hot pixel can own every event) is walked by the
// whole wave: 64 lanes gather and form 64 consecutive addends at once -- that is where the time goes, one dependent load chain
// per event -- and the sum is then taken over the lanes IN LANE ORDER, one add per event, exactly the serial order (every lane
// computes the same sum from wave-uniform reads; the owner keeps it).  Same adds, same order, same bits as the lane's own walk.
constexpr uint32_t kLongRun = 64;

template <int MODE>
__global__ void grid_accumulate(const float *__restrict__ xs, const float *__restrict__ ys, const float *__restrict__ ts,
                                const float *__restrict__ ps, int64_t n, const uint32_t *__restrict__ perm,
                                const uint32_t *__restrict__ seg, const int64_t *__restrict__ bounds, int bins, int H, int W,
                                float *__restrict__ out) {
    const int64_t pix = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const int64_t P = (int64_t)H * W;
    const bool valid = pix < P;                  // (no early return: the wave walks long runs together)
    uint32_t s = 0, e = 0;
    if (valid) s = seg[pix], e = seg[pix + 1];
    PlaneCtx c;
    c.b = blockIdx.y, c.H = H, c.W = W, c.beg = 0, c.end = 0, c.t0 = 0.f, c.dt = 1.f, c.empty = false;
    c.scale = (float)(bins - 1), c.fb = (float)c.b;
    if (MODE == EBFI_GRID_VOXEL_BILINEAR) {
        c.t0 = ts[0];
        const float tl = ts[n - 1];
        c.empty = c.t0 == 0.f && tl == 0.f;
        c.dt = (tl - c.t0) + 1e-6f;
    }
    if (MODE == EBFI_GRID_VOXEL_NAIVE) c.beg = bounds[2 * c.b], c.end = bounds[2 * c.b + 1];
    float acc = 0.f;
    if (MODE == EBFI_GRID_MASK) {
        if (e > s) {                                       // accumulate=False with duplicates: the last writer wins
            const uint32_t i = perm[e - 1];
            acc = fabsf(in_range(xs[i], ys[i], H, W) ? ps[i] : 0.f);
        }
    } else {
        const bool is_long = e - s >= kLongRun;
        if (!is_long) {
            for (uint32_t j = s; j < e; ++j) {
                float a;
                if (grid_addend<MODE>(perm[j], c, xs, ys, ts, ps, &a)) acc = acc + a;
            }
        }
        const int lane = threadIdx.x & 63;
        unsigned long long todo = __ballot(is_long);       // wave-uniform from here on
        while (todo) {
            const int owner = __ffsll((long long)todo) - 1;
            todo &= todo - 1;
            const uint32_t ls = (uint32_t)__shfl((int)s, owner), le = (uint32_t)__shfl((int)e, owner);
            float run = 0.f;
            for (uint32_t j = ls; j < le; j += 64) {
                const uint32_t cnt = le - j < 64u ? le - j : 64u;
                float a = 0.f;
                int has = 0;
                if ((uint32_t)lane < cnt) has = grid_addend<MODE>(perm[j + lane], c, xs, ys, ts, ps, &a) ? 1 : 0;
                for (uint32_t k = 0; k < cnt; ++k) {       // lane order == event order
                    const float ak = __shfl(a, (int)k);
                    if (__shfl(has, (int)k)) run = run + ak;
                }
            }
            if (lane == owner) acc = run;
        }
    }
    if (valid) out[(int64_t)c.b * P + pix] = acc;
}

// interpolate_to_image: four index_put_ in turn, so a pixel's sum is its old value, then every top-left addend in event order,
// then the top-right, bottom-left and bottom-right ones (encodings.py:12-15); each addend left to right in fp32.
// img [H, W]; keys over the same H x W (base pixels reach W - 2, H - 2).
__global__ void bilinear_accumulate(const float *__restrict__ dxs, const float *__restrict__ dys, const float *__restrict__ ws,
                                    const uint32_t *__restrict__ perm, const uint32_t *__restrict__ seg, int H, int W,
                                    float *__restrict__ img) {
    const int64_t pix = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (pix >= (int64_t)H * W) return;
    const int y = (int)(pix / W), x = (int)(pix % W);
    float acc = img[pix];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const int by = y - (c >> 1), bx = x - (c & 1);
        if (by < 0 || bx < 0) continue;
        const int64_t base = (int64_t)by * W + bx;
        const uint32_t s = seg[base], e = seg[base + 1];
        for (uint32_t j = s; j < e; ++j) {
            const uint32_t i = perm[j];
            const float dx = dxs[i], dy = dys[i];
            const float fx = (c & 1) ? dx : 1.f - dx;
            const float fy = (c >> 1) ? dy : 1.f - dy;
            acc = acc + ws[i] * fx * fy;
        }
    }
    img[pix] = acc;
}

// ------------------------------------------------------------------ hot-pixel mask, stack2cnt, polarity mask
// a beats b in torch.argmax's order: a NaN is the maximum, the first flat index wins a tie
__device__ __forceinline__ bool argmax_better(float av, int64_t ai, float bv, int64_t bi) {
    const bool an = av != av, bn = bv != bv;
    if (an != bn) return an;
    if (!an && av != bv) return av > bv;
    return ai < bi;
}

__global__ void hot_event_mask(float *__restrict__ rate, int64_t P, int max_px, float max_rate, float *__restrict__ mask) {
    __shared__ float sv[1024];
    __shared__ int64_t si[1024];
    __shared__ int stop;
    const int t = threadIdx.x, nt = blockDim.x;
    for (int64_t i = t; i < P; i += nt) mask[i] = 1.f;
    if (t == 0) stop = 0;
    __syncthreads();
    for (int round = 0; round < max_px; ++round) {
        float bv = 0.f;
        int64_t bi = -1;
        for (int64_t i = t; i < P; i += nt) {
            const float v = rate[i];
            if (bi < 0 || argmax_better(v, i, bv, bi)) bv = v, bi = i;
        }
        sv[t] = bv;
        si[t] = bi;
        __syncthreads();
        for (int d = nt >> 1; d > 0; d >>= 1) {
            if (t < d && si[t + d] >= 0 && (si[t] < 0 || argmax_better(sv[t + d], si[t + d], sv[t], si[t]))) {
                sv[t] = sv[t + d];
                si[t] = si[t + d];
            }
            __syncthreads();
        }
        if (t == 0) {
            if (si[0] >= 0 && sv[0] > max_rate) {       // a NaN maximum compares false: the loop stops, as the reference's does
                rate[si[0]] = 0.f;
                mask[si[0]] = 0.f;
            } else {
                stop = 1;
            }
        }
        __syncthreads();
        if (stop) break;
    }
}

// stack [B, TB, plane] -> cnt [B, 2, plane]: round half to even, then the positive and the negated negative parts summed over
// the bin axis in bin order
__global__ void stack_to_cnt(const float *__restrict__ stack, int64_t B, int TB, int64_t plane, float *__restrict__ cnt) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= B * plane) return;
    const int64_t b = i / plane, q = i % plane;
    const float *src = stack + b * TB * plane + q;
    float pos = 0.f, neg = 0.f;
    for (int t = 0; t < TB; ++t) {
        const float r = rintf(src[(int64_t)t * plane]);
        pos = pos + (r < 0.f ? 0.f : r);
        neg = neg + (r > 0.f ? 0.f : r) * -1.f;
    }
    cnt[(b * 2) * plane + q] = pos;
    cnt[(b * 2 + 1) * plane + q] = neg;
}

// out [2, n]: row 0 = ps with the negatives zeroed, row 1 = -(ps with the positives zeroed)
__global__ void polarity_mask(const float *__restrict__ ps, int64_t n, float *__restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const float p = ps[i];
    out[i] = p < 0.f ? 0.f : p;
    out[n + i] = (p > 0.f ? 0.f : p) * -1.f;
}

// ------------------------------------------------------------------ host side
constexpr size_t kAlign = 256;
static inline size_t up(size_t v) { return (v + kAlign - 1) / kAlign * kAlign; }

struct Layout {
    size_t keys[2], perm[2], hist, sums, seg, bounds, pxs, pys, dxs, dys, ws, total;
    int64_t nb, m, nt;
};

// n >= 0, bins >= 1, P >= 1 checked by the callers
Layout layout(int64_t n, int bins, int64_t P) {
    Layout L;
    L.nb = ceil_div(n, kBlock);
    L.m = 256 * L.nb;
    L.nt = ceil_div(L.m, kScanTile);
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
    L.seg = take((size_t)(P + 2) * 4);
    L.bounds = take((size_t)(2 * bins + 1) * 8);
    L.pxs = take((size_t)n * 8);
    L.pys = take((size_t)n * 8);
    L.dxs = take((size_t)n * 4);
    L.dys = take((size_t)n * 4);
    L.ws = take((size_t)n * 4);
    L.total = at;
    return L;
}

constexpr int64_t kMaxEvents = ((int64_t)1 << 31) - 1 - kBlock;       // permutation entries and table sums are uint32
constexpr int64_t kMaxPixels = ((int64_t)1 << 31) - 2;

int sizes_ok(const char *what, int64_t n, int bins, int H, int W) {
    if (n < 0 || bins < 1 || H < 1 || W < 1) return fail(EBFI_ERR_ARG, "%s: bad sizes", what);
    if (n > kMaxEvents || (int64_t)H * W > kMaxPixels || bins > 65535)
        return fail(EBFI_ERR_UNSUPPORTED, "%s: more than 2^31 - 257 events, 2^31 - 2 pixels or 65535 planes", what);
    return EBFI_OK;
}

// keys in ws + L.keys[0] -> sorted keys / permutation (returned through the pointers) and seg[0 .. nkeys]
int build_index(char *ws, const Layout &L, int64_t n, int64_t nkeys, hipStream_t st, const uint32_t **perm_out,
                const uint32_t **seg_out) {
    uint32_t *keys[2] = {reinterpret_cast<uint32_t *>(ws + L.keys[0]), reinterpret_cast<uint32_t *>(ws + L.keys[1])};
    uint32_t *perm[2] = {reinterpret_cast<uint32_t *>(ws + L.perm[0]), reinterpret_cast<uint32_t *>(ws + L.perm[1])};
    uint32_t *hist = reinterpret_cast<uint32_t *>(ws + L.hist), *sums = reinterpret_cast<uint32_t *>(ws + L.sums);
    uint32_t *seg = reinterpret_cast<uint32_t *>(ws + L.seg);
    int bits = 0;
    while (bits < 32 && ((uint64_t)nkeys >> bits) != 0) ++bits;       // keys lie in [0, nkeys]
    const int passes = bits == 0 ? 1 : (bits + 7) / 8;
    int cur = 0;
    for (int p = 0; p < passes; ++p) {
        const int shift = 8 * p;
        {
            ProfScope ps_("enc_sort_hist", st);
            hipLaunchKernelGGL(sort_hist, dim3((unsigned)L.nb), dim3(kBlock), 0, st, keys[cur], n, shift, hist, (int)L.nb);
        }
        if (int rc = check_launch("enc_sort_hist")) return rc;
        {
            ProfScope ps_("enc_scan_tiles", st);
            hipLaunchKernelGGL(scan_tiles, dim3((unsigned)L.nt), dim3(kBlock), 0, st, hist, L.m, sums);
        }
        if (int rc = check_launch("enc_scan_tiles")) return rc;
        {
            ProfScope ps_("enc_scan_sums", st);
            hipLaunchKernelGGL(scan_sums, dim3(1), dim3(kBlock), 0, st, sums, L.nt);
        }
        if (int rc = check_launch("enc_scan_sums")) return rc;
        {
            ProfScope ps_("enc_sort_scatter", st);
            hipLaunchKernelGGL(sort_scatter, dim3((unsigned)L.nb), dim3(kBlock), 0, st, keys[cur],
                               p == 0 ? (const uint32_t *)nullptr : perm[cur], n, shift, hist, sums, (int)L.nb, keys[cur ^ 1],
                               perm[cur ^ 1]);
        }
        if (int rc = check_launch("enc_sort_scatter")) return rc;
        cur ^= 1;
    }
    {
        ProfScope ps_("enc_grid_segments", st);
        hipLaunchKernelGGL(grid_segments, dim3((unsigned)ceil_div(nkeys + 1, kBlock)), dim3(kBlock), 0, st, keys[cur], n, nkeys,
                           seg);
    }
    if (int rc = check_launch("enc_grid_segments")) return rc;
    *perm_out = perm[cur];
    *seg_out = seg;
    return EBFI_OK;
}

int run_bilinear(const int64_t *pxs, const int64_t *pys, const float *dxs, const float *dys, const float *w, int64_t n, int H,
                 int W, float *img, char *ws, const Layout &L, hipStream_t st) {
    const int64_t P = (int64_t)H * W;
    {
        ProfScope ps_("enc_bilinear_keys", st);
        hipLaunchKernelGGL(bilinear_keys, dim3((unsigned)L.nb), dim3(kBlock), 0, st, pxs, pys, n, H, W,
                           reinterpret_cast<uint32_t *>(ws + L.keys[0]));
    }
    if (int rc = check_launch("enc_bilinear_keys")) return rc;
    const uint32_t *perm, *seg;
    if (int rc = build_index(ws, L, n, P, st, &perm, &seg)) return rc;
    {
        ProfScope ps_("enc_bilinear_accumulate", st);
        hipLaunchKernelGGL(bilinear_accumulate, dim3((unsigned)ceil_div(P, kBlock)), dim3(kBlock), 0, st, dxs, dys, w, perm, seg,
                           H, W, img);
    }
    return check_launch("enc_bilinear_accumulate");
}

}  // namespace

extern "C" int64_t ebfi_events_grid_workspace(int64_t n, int bins, int H, int W) {
    if (n < 0 || bins < 1 || H < 1 || W < 1 || n > kMaxEvents || (int64_t)(H + 1) * (W + 1) > kMaxPixels) return 0;
    return (int64_t)layout(n, bins, (int64_t)(H + 1) * (W + 1)).total;      // (the padded bilinear image is the largest grid)
}

extern "C" int ebfi_events_to_grid(const float *xs, const float *ys, const float *ts, const float *ps, int64_t n, int mode,
                                   int bins, int H, int W, float *out, void *workspace, int64_t workspace_bytes, void *stream) {
    if (int rc = sizes_ok("events_to_grid", n, bins, H, W)) return rc;
    if (mode < EBFI_GRID_IMAGE || mode > EBFI_GRID_BILINEAR_CLIPPED) return fail(EBFI_ERR_ARG, "events_to_grid: unknown mode %d", mode);
    const bool timed = mode == EBFI_GRID_VOXEL_BILINEAR || mode == EBFI_GRID_VOXEL_NORMALISED || mode == EBFI_GRID_VOXEL_NAIVE ||
                       mode == EBFI_GRID_STACK_NO_POLARITY;
    const bool bilinear = mode == EBFI_GRID_BILINEAR_PADDED || mode == EBFI_GRID_BILINEAR_CLIPPED;
    if (!timed && bins != (mode == EBFI_GRID_CHANNELS ? 2 : 1))
        return fail(EBFI_ERR_ARG, "events_to_grid: this mode writes %d plane(s), bins must say so", mode == EBFI_GRID_CHANNELS ? 2 : 1);
    if (!out) return fail(EBFI_ERR_ARG, "events_to_grid: null output");
    if (n > 0 && (!xs || !ys || !ps || (timed && !ts))) return fail(EBFI_ERR_ARG, "events_to_grid: null event array");
    if ((int64_t)(H + 1) * (W + 1) > kMaxPixels) return fail(EBFI_ERR_UNSUPPORTED, "events_to_grid: more than 2^31 - 2 pixels");
    const int oH = H + (mode == EBFI_GRID_BILINEAR_PADDED), oW = W + (mode == EBFI_GRID_BILINEAR_PADDED);
    const int64_t P = (int64_t)oH * oW;
    const int64_t need = ebfi_events_grid_workspace(n, bins, H, W);
    if (!workspace || workspace_bytes < need) return fail(EBFI_ERR_WORKSPACE, "events_to_grid: workspace too small");
    if (reinterpret_cast<uintptr_t>(workspace) % 16) return fail(EBFI_ERR_ARG, "events_to_grid: workspace not 16-byte aligned");
    hipStream_t st = static_cast<hipStream_t>(stream);
    // nothing to add (and, for the two voxel_torch forms and the stack, the reference's own `len(ts) <= 3` exit): zeros
    const bool short_list = mode == EBFI_GRID_VOXEL_BILINEAR || mode == EBFI_GRID_VOXEL_NAIVE || mode == EBFI_GRID_STACK_NO_POLARITY;
    if (n == 0 || (short_list && n <= 3)) {
        if (hipMemsetAsync(out, 0, (size_t)bins * P * sizeof(float), st) != hipSuccess)
            return fail(EBFI_ERR_LAUNCH, "events_to_grid: memset failed");
        return EBFI_OK;
    }
    char *ws = static_cast<char *>(workspace);
    const Layout L = layout(n, bins, (int64_t)(H + 1) * (W + 1));
    if (bilinear) {
        int64_t *pxs = reinterpret_cast<int64_t *>(ws + L.pxs), *pys = reinterpret_cast<int64_t *>(ws + L.pys);
        float *dxs = reinterpret_cast<float *>(ws + L.dxs), *dys = reinterpret_cast<float *>(ws + L.dys);
        float *w = reinterpret_cast<float *>(ws + L.ws);
        if (hipMemsetAsync(out, 0, (size_t)P * sizeof(float), st) != hipSuccess)
            return fail(EBFI_ERR_LAUNCH, "events_to_grid: memset failed");
        {
            ProfScope ps_("enc_bilinear_prepare", st);
            hipLaunchKernelGGL(bilinear_prepare, dim3((unsigned)L.nb), dim3(kBlock), 0, st, xs, ys, ps, n, H, W,
                               (int)(mode == EBFI_GRID_BILINEAR_PADDED), pxs, pys, dxs, dys, w);
        }
        if (int rc = check_launch("enc_bilinear_prepare")) return rc;
        return run_bilinear(pxs, pys, dxs, dys, w, n, oH, oW, out, ws, L, st);
    }
    {
        ProfScope ps_("enc_grid_keys", st);
        hipLaunchKernelGGL(grid_keys, dim3((unsigned)L.nb), dim3(kBlock), 0, st, xs, ys, n, H, W,
                           reinterpret_cast<uint32_t *>(ws + L.keys[0]));
    }
    if (int rc = check_launch("enc_grid_keys")) return rc;
    const uint32_t *perm, *seg;
    if (int rc = build_index(ws, L, n, P, st, &perm, &seg)) return rc;
    int64_t *bounds = reinterpret_cast<int64_t *>(ws + L.bounds);
    if (mode == EBFI_GRID_VOXEL_NAIVE || mode == EBFI_GRID_STACK_NO_POLARITY) {
        {
            ProfScope ps_("enc_grid_bounds", st);
            hipLaunchKernelGGL(grid_bounds, dim3((unsigned)ceil_div(bins, 64)), dim3(64), 0, st, ts, n, bins, bounds);
        }
        if (int rc = check_launch("enc_grid_bounds")) return rc;
    }
    const dim3 grid((unsigned)ceil_div(P, kBlock), (unsigned)bins), block(kBlock);
    ProfScope ps_("enc_grid_accumulate", st);
#define EBFI_GRID_LAUNCH(M) \
    hipLaunchKernelGGL(grid_accumulate<M>, grid, block, 0, st, xs, ys, ts, ps, n, perm, seg, bounds, bins, H, W, out)
    switch (mode) {
        case EBFI_GRID_IMAGE: EBFI_GRID_LAUNCH(EBFI_GRID_IMAGE); break;
        case EBFI_GRID_MASK: EBFI_GRID_LAUNCH(EBFI_GRID_MASK); break;
        case EBFI_GRID_CHANNELS: EBFI_GRID_LAUNCH(EBFI_GRID_CHANNELS); break;
        case EBFI_GRID_VOXEL_BILINEAR: EBFI_GRID_LAUNCH(EBFI_GRID_VOXEL_BILINEAR); break;
        case EBFI_GRID_VOXEL_NORMALISED: EBFI_GRID_LAUNCH(EBFI_GRID_VOXEL_NORMALISED); break;
        default: EBFI_GRID_LAUNCH(EBFI_GRID_VOXEL_NAIVE); break;
    }
#undef EBFI_GRID_LAUNCH
    return check_launch("enc_grid_accumulate");
}

extern "C" int ebfi_interpolate_to_image(const int64_t *pxs, const int64_t *pys, const float *dxs, const float *dys,
                                         const float *weights, int64_t n, int H, int W, float *img, void *workspace,
                                         int64_t workspace_bytes, void *stream) {
    if (int rc = sizes_ok("interpolate_to_image", n, 1, H, W)) return rc;
    if (!img) return fail(EBFI_ERR_ARG, "interpolate_to_image: null image");
    if (n > 0 && (!pxs || !pys || !dxs || !dys || !weights)) return fail(EBFI_ERR_ARG, "interpolate_to_image: null event array");
    if (n == 0) return EBFI_OK;
    const int64_t need = ebfi_events_grid_workspace(n, 1, H, W);
    if (need == 0) return fail(EBFI_ERR_UNSUPPORTED, "interpolate_to_image: more than 2^31 - 2 pixels");
    if (!workspace || workspace_bytes < need) return fail(EBFI_ERR_WORKSPACE, "interpolate_to_image: workspace too small");
    if (reinterpret_cast<uintptr_t>(workspace) % 16) return fail(EBFI_ERR_ARG, "interpolate_to_image: workspace not 16-byte aligned");
    const Layout L = layout(n, 1, (int64_t)(H + 1) * (W + 1));
    return run_bilinear(pxs, pys, dxs, dys, weights, n, H, W, img, static_cast<char *>(workspace), L,
                        static_cast<hipStream_t>(stream));
}

extern "C" int ebfi_hot_event_mask(float *event_rate, int H, int W, int max_px, float max_rate, float *mask, void *stream) {
    if (H < 1 || W < 1 || max_px < 0) return fail(EBFI_ERR_ARG, "hot_event_mask: bad sizes");
    if (!event_rate || !mask) return fail(EBFI_ERR_ARG, "hot_event_mask: null pointer");
    hipStream_t st = static_cast<hipStream_t>(stream);
    ProfScope ps_("enc_hot_event_mask", st);
    hipLaunchKernelGGL(hot_event_mask, dim3(1), dim3(1024), 0, st, event_rate, (int64_t)H * W, max_px, max_rate, mask);
    return check_launch("enc_hot_event_mask");
}

extern "C" int ebfi_stack_to_cnt(const float *stack, int64_t B, int TB, int64_t plane, float *cnt, void *stream) {
    if (B < 0 || TB < 0 || plane < 0) return fail(EBFI_ERR_ARG, "stack_to_cnt: bad sizes");
    if (B == 0 || plane == 0) return EBFI_OK;
    if (!cnt || (TB > 0 && !stack)) return fail(EBFI_ERR_ARG, "stack_to_cnt: null pointer");
    if (plane > kMaxPixels || B > kMaxPixels / plane * kBlock) return fail(EBFI_ERR_UNSUPPORTED, "stack_to_cnt: grid beyond 2^31 - 1");
    hipStream_t st = static_cast<hipStream_t>(stream);
    ProfScope ps_("enc_stack_to_cnt", st);
    hipLaunchKernelGGL(stack_to_cnt, dim3((unsigned)ceil_div(B * plane, kBlock)), dim3(kBlock), 0, st, stack, B, TB, plane, cnt);
    return check_launch("enc_stack_to_cnt");
}

extern "C" int ebfi_polarity_mask(const float *ps, int64_t n, float *out, void *stream) {
    if (n < 0) return fail(EBFI_ERR_ARG, "polarity_mask: bad size");
    if (n == 0) return EBFI_OK;
    if (!ps || !out) return fail(EBFI_ERR_ARG, "polarity_mask: null pointer");
    if (n > kMaxEvents) return fail(EBFI_ERR_UNSUPPORTED, "polarity_mask: more than 2^31 - 257 values");
    hipStream_t st = static_cast<hipStream_t>(stream);
    ProfScope ps_("enc_polarity_mask", st);
    hipLaunchKernelGGL(polarity_mask, dim3((unsigned)ceil_div(n, kBlock)), dim3(kBlock), 0, st, ps, n, out);
    return check_launch("enc_polarity_mask");
}
