// The device noise law of the clip loaders: AugmentData's crop, flips, add_noise and add_hot_pixels on an event stack
// (dataloader/h5dataset.py:368-463) in one pass from the binned stack to the item's final stack, plus the hot pixels in place.
//
// The host law (ebfi_amd.clipdata.draw_noise) is the reference's bit for bit: a sequential MT19937 stream through torch's CPU
// normal transform, 11 to 73 ms per 16 x 2 x 256 x 256 item by the host (profiles/loader_real_data.md).  This file is a second law with the same distribution that a
// GPU can draw: everything random is a function of (seed, cell) through a counter-based generator, and nothing in it is
// floating point, so tests/eventaug_ref.py restates it in numpy to the bit.
//
//   generator   Philox4x32-10 (Salmon et al., SC'11): key = the 64-bit seed, counter = (group low, group high, stream, 0).
//               Stream 0 is the noise field -- cell c takes word c & 3 of group c >> 2 -- stream 1 the hot pixels.
//   count       k = #{m : u < table[m]} of a draw's word u; table[m] = floor(2^32 f erfc((m + 1) / (std sqrt 2))) comes from the
//               host in float64 and is strictly decreasing, so P(k >= m) = f P(|N(0, std)| >= m): the distribution of
//               int(|N(0, std)|) on a fraction f of the cells.  The table travels by value in the kernel arguments and is read
//               through scalar loads (its index is uniform); no transcendental runs here.
//
// event_augment: a thread owns FOUR consecutive cells of the contiguous destination, i.e. one Philox call when the item starts
// at a group boundary (two when a load of a multi-load item does not) and one 16-byte store.  Its four cells usually lie in one
// row of the window; then their source is four consecutive floats (read backwards under a horizontal flip) and goes through one
// 16-byte load when that address happens to be 16-byte aligned -- decided per thread from the address itself, so no window
// origin, stride or storage offset is assumed.  Cells that straddle a row end, or an unaligned source, take four scalar loads
// with the (plane, row, column) odometer advanced by hand.  The index arithmetic is one 64-bit division per thread (cell ->
// plane), the rest is 32-bit: h * w < 2^31 is checked on the host.
//
// Arithmetic per four cells is ten Philox rounds (four 32 x 32 -> 64 multiplies each) plus table_len compares per cell against
// 32 bytes of traffic: ALU and HBM time are of the same order, a few microseconds for a 2M-cell item either way (measured:
// 7.2 us without a table, 9.3 us with the seven entries of std 1.0, profiles/loader_real_data.md).
#include "common.hpp"

using namespace ebfi;

namespace {

constexpr int kThreads = 256;
constexpr int kCells = 4;   // cells per thread = words per Philox call

struct NoiseTable {
    uint32_t n;
    uint32_t t[EBFI_NOISE_TABLE_MAX];
};

struct Words4 {
    uint32_t v[4];
};

__device__ inline Words4 philox4x32_10(uint64_t group, uint32_t stream, uint64_t seed) {
    uint32_t c0 = (uint32_t)group, c1 = (uint32_t)(group >> 32), c2 = stream, c3 = 0u;
    uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c1 = (uint32_t)p1;
        c3 = (uint32_t)p0;
        c0 = n0;
        c2 = n2;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    return Words4{{c0, c1, c2, c3}};
}

__device__ inline uint32_t count_of(uint32_t u, const NoiseTable &tab) {
    uint32_t k = 0;
    for (uint32_t m = 0; m < tab.n; ++m) k += u < tab.t[m] ? 1u : 0u;   // (uniform bound and index: scalar loads)
    return k;
}

// the last, partial quad of a stack whose size is no multiple of four.  Kept out of line: inlined beside the 16-byte store the
// compiler merges the two branches' stores and splits the vector store into a 12-byte and a 4-byte one
__device__ __attribute__((noinline)) void store_tail(float *__restrict__ p, float4 o, int live) {
    p[0] = o.x;
    if (live > 1) p[1] = o.y;
    if (live > 2) p[2] = o.z;
}

// VEC: dst is 16-byte aligned (every full quad goes out as one float4)
template <bool VEC>
__global__ __launch_bounds__(kThreads) void event_augment(const float *__restrict__ src, int64_t sb, int64_t sp, int64_t sr,
                                                          int64_t total, int i0, int j0, int h, int w, int fliph, int flipv,
                                                          uint64_t seed, NoiseTable tab, int64_t cell0,
                                                          float *__restrict__ dst) {
    const uint32_t plane = (uint32_t)h * (uint32_t)w;
    const int64_t quads = (total + kCells - 1) / kCells;
    const uint32_t lane0 = (uint32_t)(cell0 & 3);   // where this call's first cell sits in its Philox group
    for (int64_t t = (int64_t)blockIdx.x * kThreads + threadIdx.x; t < quads; t += (int64_t)gridDim.x * kThreads) {
        const int64_t c = t * kCells;
        const int live = total - c < kCells ? (int)(total - c) : kCells;
        // ---- the four counts
        uint32_t k[kCells] = {0u, 0u, 0u, 0u};
        if (tab.n) {
            const uint64_t g = (uint64_t)(cell0 + c) >> 2;
            Words4 a = philox4x32_10(g, 0u, seed);
            if (lane0) {   // (uniform) the quad straddles two groups
                const Words4 b = philox4x32_10(g + 1, 0u, seed);
                uint32_t both[8];
#pragma unroll
                for (int q = 0; q < 4; ++q) both[q] = a.v[q], both[4 + q] = b.v[q];
#pragma unroll
                for (int q = 0; q < 4; ++q) a.v[q] = lane0 == 1 ? both[q + 1] : lane0 == 2 ? both[q + 2] : both[q + 3];
            }
#pragma unroll
            for (int q = 0; q < kCells; ++q) k[q] = count_of(a.v[q], tab);
        }
        // ---- the four source values
        const int64_t pl = c / plane;                          // b * 2 + p
        const uint32_t rem = (uint32_t)(c - pl * plane);
        int y = (int)(rem / (uint32_t)w), x = (int)(rem % (uint32_t)w);
        const float *base = src + (pl >> 1) * sb + (pl & 1) * sp;
        float v[kCells] = {0.0f, 0.0f, 0.0f, 0.0f};
        bool done = false;
        if (live == kCells && x + kCells <= w) {
            const int Y = i0 + (flipv ? h - 1 - y : y);
            const int X0 = fliph ? j0 + w - kCells - x : j0 + x;   // lowest source column of the four
            const float *p = base + (int64_t)Y * sr + X0;
            if ((reinterpret_cast<uintptr_t>(p) & 15u) == 0) {
                const float4 f = *reinterpret_cast<const float4 *>(p);
                v[0] = fliph ? f.w : f.x;
                v[1] = fliph ? f.z : f.y;
                v[2] = fliph ? f.y : f.z;
                v[3] = fliph ? f.x : f.w;
                done = true;
            }
        }
        if (!done) {
            int64_t pq = pl;
#pragma unroll
            for (int q = 0; q < kCells; ++q) {
                if (q < live) {
                    const int Y = i0 + (flipv ? h - 1 - y : y);
                    const int X = j0 + (fliph ? w - 1 - x : x);
                    v[q] = src[(pq >> 1) * sb + (pq & 1) * sp + (int64_t)Y * sr + X];
                    if (++x == w) {
                        x = 0;
                        if (++y == h) y = 0, ++pq;
                    }
                }
            }
        }
        // ---- store
        float4 o;
        o.x = v[0] + (float)k[0];
        o.y = v[1] + (float)k[1];
        o.z = v[2] + (float)k[2];
        o.w = v[3] + (float)k[3];
        if (live < kCells) {
            store_tail(dst + c, o, live);
        } else if constexpr (VEC) {
            *reinterpret_cast<float4 *>(dst + c) = o;
        } else {
            dst[c] = o.x;
            dst[c + 1] = o.y;
            dst[c + 2] = o.z;
            dst[c + 3] = o.w;
        }
    }
}

// one thread per (hot pixel, plane), the plane the fast index: the Philox call is repeated per plane (cheaper than a second
// pass or a table of positions), the adds are float atomics of small integers -- exact, so their order does not matter
__global__ __launch_bounds__(kThreads) void event_hot_pixels(float *__restrict__ stack, int64_t planes, int h, int w,
                                                             uint64_t seed, NoiseTable tab, int64_t n_hot) {
    const int64_t total = planes * n_hot;
    const int64_t plane = (int64_t)h * w;
    for (int64_t t = (int64_t)blockIdx.x * kThreads + threadIdx.x; t < total; t += (int64_t)gridDim.x * kThreads) {
        const int64_t n = t / planes, pl = t - n * planes;
        const Words4 u = philox4x32_10((uint64_t)n, 1u, seed);
        const uint32_t k = count_of(u.v[2], tab);
        if (k == 0) continue;
        const uint32_t x = (uint32_t)(((uint64_t)u.v[0] * (uint32_t)w) >> 32);   // < w
        const uint32_t y = (uint32_t)(((uint64_t)u.v[1] * (uint32_t)h) >> 32);   // < h
        atomicAdd(stack + pl * plane + (int64_t)y * w + x, (float)k);
    }
}

inline unsigned grid_for(int64_t threads) {
    const int64_t blocks = ceil_div(threads, kThreads);
    return (unsigned)(blocks < (1 << 20) ? blocks : (1 << 20));   // (grid-stride loops cover the rest)
}

// 0 or an error code; fills `tab`
int load_table(const char *who, const uint32_t *table, int table_len, NoiseTable &tab) {
    if (table_len < 0 || table_len > EBFI_NOISE_TABLE_MAX)
        return fail(EBFI_ERR_ARG, "%s: table_len %d outside [0, %d]", who, table_len, EBFI_NOISE_TABLE_MAX);
    if (table_len > 0 && !table) return fail(EBFI_ERR_ARG, "%s: null pointer (table)", who);
    tab.n = (uint32_t)table_len;
    for (int m = 0; m < EBFI_NOISE_TABLE_MAX; ++m) tab.t[m] = m < table_len ? table[m] : 0u;
    return EBFI_OK;
}

}  // namespace

extern "C" int ebfi_event_augment(const float *src, const int64_t src_strides[3], int64_t TB, int H0, int W0, int i, int j,
                                  int h, int w, int flip_h, int flip_v, uint64_t seed, const uint32_t *table, int table_len,
                                  int64_t cell_offset, float *dst, void *stream) {
    if (!src || !dst || !src_strides) return fail(EBFI_ERR_ARG, "event_augment: null pointer");
    if (TB < 1 || TB > (1 << 24) || H0 < 1 || W0 < 1)
        return fail(EBFI_ERR_ARG, "event_augment: bad sizes TB=%lld H0=%d W0=%d", (long long)TB, H0, W0);
    if (i < 0 || j < 0 || h < 1 || w < 1 || (int64_t)i + h > H0 || (int64_t)j + w > W0)
        return fail(EBFI_ERR_ARG, "event_augment: window (%d, %d, %d, %d) outside the %d x %d frame", i, j, h, w, H0, W0);
    if ((int64_t)h * w >= ((int64_t)1 << 31))
        return fail(EBFI_ERR_ARG, "event_augment: window of %d x %d cells (a plane must stay below 2^31)", h, w);
    const int64_t sb = src_strides[0], sp = src_strides[1], sr = src_strides[2];
    if (sb < 0 || sp < 0 || sr < 0) return fail(EBFI_ERR_ARG, "event_augment: strides must be >= 0");
    if ((double)(TB - 1) * (double)sb + (double)sp + (double)(H0 - 1) * (double)sr + (double)W0 > 0x1p60)
        return fail(EBFI_ERR_ARG, "event_augment: strides reach past 2^60 elements");
    if (cell_offset < 0 || cell_offset > ((int64_t)1 << 60))
        return fail(EBFI_ERR_ARG, "event_augment: cell_offset %lld outside [0, 2^60]", (long long)cell_offset);
    NoiseTable tab;
    if (int rc = load_table("event_augment", table, table_len, tab)) return rc;
    const int64_t total = TB * 2 * (int64_t)h * w;
    // the ranges the kernel may touch, in bytes: the source up to its last readable element, the destination's `total` floats
    const int64_t span = (TB - 1) * sb + sp + (int64_t)(H0 - 1) * sr + W0;
    const uintptr_t s0 = reinterpret_cast<uintptr_t>(src), s1 = s0 + (uintptr_t)span * sizeof(float);
    const uintptr_t d0 = reinterpret_cast<uintptr_t>(dst), d1 = d0 + (uintptr_t)total * sizeof(float);
    if (s0 < d1 && d0 < s1) return fail(EBFI_ERR_ARG, "event_augment: source and destination overlap");
    hipStream_t st = static_cast<hipStream_t>(stream);
    const dim3 grid(grid_for(ceil_div(total, kCells))), block(kThreads);
    {
        ProfScope ps_("event_augment", st, 0.0, (double)total * 8.0);
        if (aligned16(dst))
            hipLaunchKernelGGL((event_augment<true>), grid, block, 0, st, src, sb, sp, sr, total, i, j, h, w, flip_h, flip_v, seed,
                               tab, cell_offset, dst);
        else
            hipLaunchKernelGGL((event_augment<false>), grid, block, 0, st, src, sb, sp, sr, total, i, j, h, w, flip_h, flip_v,
                               seed, tab, cell_offset, dst);
    }
    return check_launch("event_augment");
}

extern "C" int ebfi_event_hot_pixels(float *stack, int64_t planes, int h, int w, uint64_t seed, const uint32_t *table,
                                     int table_len, int64_t n_hot, void *stream) {
    if (!stack) return fail(EBFI_ERR_ARG, "event_hot_pixels: null pointer");
    if (planes < 1 || h < 1 || w < 1 || (int64_t)h * w >= ((int64_t)1 << 31))
        return fail(EBFI_ERR_ARG, "event_hot_pixels: bad sizes planes=%lld h=%d w=%d", (long long)planes, h, w);
    if (n_hot < 0 || planes >= ((int64_t)1 << 40) || n_hot >= ((int64_t)1 << 40) / planes)
        return fail(EBFI_ERR_ARG, "event_hot_pixels: n_hot=%lld on %lld planes (planes * n_hot must stay below 2^40)",
                    (long long)n_hot, (long long)planes);
    NoiseTable tab;
    if (int rc = load_table("event_hot_pixels", table, table_len, tab)) return rc;
    if (n_hot == 0 || table_len == 0) return EBFI_OK;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const dim3 grid(grid_for(planes * n_hot)), block(kThreads);
    {
        ProfScope ps_("event_hot_pixels", st, 0.0, (double)planes * n_hot * 8.0);
        hipLaunchKernelGGL(event_hot_pixels, grid, block, 0, st, stack, planes, h, w, seed, tab, n_hot);
    }
    return check_launch("event_hot_pixels");
}
