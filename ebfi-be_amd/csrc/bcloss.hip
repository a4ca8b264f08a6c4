// loss/reconstruction.py (BrightnessConstancy) and myutils/gradients.py (Sobel) on the device: the generative-model term, the
// temporal-consistency term, the total-variation term and the Sobel operator, each with its gradients.
//
// THE LAW.  A pixel (b, h, w) with flow (fx, fy) -- channel 0 horizontal, channel 1 vertical, in units of S = max(H, W) --
// samples at ix = ((gx + 1) * W - 1) / 2 with gx = 2 * (w - fx * S) / (W - 1) - 1 (grid_sample without align_corners), iy
// alike with H: bilinear, corners outside the image contribute 0.  The coordinate and the per-pixel arithmetic are float64 of
// the float32 inputs; the Sobel values of the (up to) four corners come from the 4 x 4 window of the image with clamped
// coordinates (the replication pad), so no Sobel image exists in the forward.  Every term writes a per-pixel residual and is
// reduced in float64 in two stages of fixed order: two launches per term.  generative_model needs a third, small one in front
// (ebfi_bc_mask_flow): AveragedIWE reads the masked flow as a tensor, and csrc/iwe.hip, whose text a host test pins, could not
// be given a mask to apply while it reads.
// The gradient into the flow is a gather (each pixel owns its element).  The gradient into the SAMPLED image is the scatter:
// entry e = 4 * source pixel + corner (top-left, top-right, bottom-left, bottom-right) carries a float32 addend and the key
// of its destination pixel (B * H * W for a corner outside the image); a stable 8-bit LSD radix sort of (key, e), run starts
// by bisection, then one thread per destination adds its run in ascending e, fp32, unfused; a run of 64 entries or more is
// gathered by the whole wave and summed over the lanes in lane order.  No float atomics, nothing read back, every launch on
// the caller's stream in one chain.  For the generative term the Sobel adjoint is then a gather from the two gradient images.
//
// The sort is a private copy of the one in csrc/iwe.hip and csrc/encodings.hip (host tests pin the text of both files).
#include "common.hpp"

#pragma clang fp contract(off)

using namespace ebfi;

namespace {

constexpr int kBlock = 256;
constexpr int kScanTile = 1024;
constexpr uint32_t kLongRun = 64;

// ------------------------------------------------------------------ stable LSD radix sort, 8 bits per pass (as iwe.hip)
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

// out [PLANES][nkeys]; val [PLANES][n]: one thread per destination key adds its run in entry order, every plane its own chain
template <int PLANES>
__global__ void accumulate(const float *__restrict__ val, int64_t n, const uint32_t *__restrict__ perm,
                           const uint32_t *__restrict__ seg, int64_t nkeys, float *__restrict__ out) {
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
            const uint32_t g = perm[j];
#pragma unroll
            for (int p = 0; p < PLANES; ++p) acc[p] = acc[p] + val[(int64_t)p * n + g];
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
            if ((uint32_t)lane < cnt) {
                const uint32_t g = perm[j + lane];
#pragma unroll
                for (int p = 0; p < PLANES; ++p) v[p] = val[(int64_t)p * n + g];
            }
            for (uint32_t k = 0; k < cnt; ++k) {      // lane order == entry order
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
    for (int p = 0; p < PLANES; ++p) out[(int64_t)p * nkeys + key] = acc[p];
}

// ------------------------------------------------------------------ the two-stage float64 sum
__device__ __forceinline__ double block_sum(double v, double *buf) {
    buf[threadIdx.x] = v;
    __syncthreads();
    for (int d = kBlock / 2; d > 0; d >>= 1) {
        if ((int)threadIdx.x < d) buf[threadIdx.x] = buf[threadIdx.x] + buf[threadIdx.x + d];
        __syncthreads();
    }
    return buf[0];
}

__global__ void loss_final(const double *__restrict__ partials, int64_t n, double weight, float *__restrict__ loss) {
    __shared__ double buf[kBlock];
    double v = 0.0;
    for (int64_t i = threadIdx.x; i < n; i += kBlock) v = v + partials[i];
    const double total = block_sum(v, buf);
    if (threadIdx.x == 0) *loss = (float)(weight * total);
}

// ------------------------------------------------------------------ the sample of one pixel
struct Flow4 {
    const float *p;
    int64_t sb, sc, sh, sw;      // strides in elements
};

struct Sample {
    int x0, y0;                  // the top-left corner (may lie one outside the image)
    double tx, ty;               // fractions: the weights are (1 - tx, tx) x (1 - ty, ty)
    bool ok;                     // finite and at least one corner can be inside
    bool in[4];                  // corner inside the image: tl, tr, bl, br
    double w[4];
};

// sample coordinate of position p (0 .. n - 1) under flow f: grid_sample's align_corners = False, not p - f * S
__device__ __forceinline__ double coordinate(int p, float f, double S, int n) {
    const double g = 2.0 * ((double)p - (double)f * S) / (double)(n - 1) - 1.0;
    return ((g + 1.0) * (double)n - 1.0) / 2.0;
}

__device__ __forceinline__ Sample sample_at(int h, int w, float fx, float fy, double S, int H, int W) {
    Sample s;
    const double ix = coordinate(w, fx, S, W), iy = coordinate(h, fy, S, H);
    // a NaN fails the comparisons; outside [-1, n) no corner is inside (and the floor fits an int inside it)
    s.ok = ix >= -1.0 && ix < (double)W && iy >= -1.0 && iy < (double)H;
    s.x0 = s.y0 = 0;
    s.tx = s.ty = 0.0;
    if (s.ok) {
        const double fx0 = floor(ix), fy0 = floor(iy);
        s.x0 = (int)fx0, s.y0 = (int)fy0;
        s.tx = ix - fx0, s.ty = iy - fy0;
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const int y = s.y0 + (c >> 1), x = s.x0 + (c & 1);
        s.in[c] = s.ok && y >= 0 && y < H && x >= 0 && x < W;
        s.w[c] = ((c & 1) ? s.tx : 1.0 - s.tx) * ((c >> 1) ? s.ty : 1.0 - s.ty);
    }
    return s;
}

__device__ __forceinline__ int clampi(int v, int n) { return v < 0 ? 0 : (v >= n ? n - 1 : v); }

// Sobel values of the four corners from the 4 x 4 window with clamped coordinates; a corner outside the image gives 0
__device__ __forceinline__ void corner_sobel(const float *__restrict__ plane, const Sample &s, int H, int W, double *sx, double *sy) {
    double win[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int y = clampi(s.y0 - 1 + i, H);
#pragma unroll
        for (int j = 0; j < 4; ++j) win[i][j] = (double)plane[(int64_t)y * W + clampi(s.x0 - 1 + j, W)];
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const int r = c >> 1, q = c & 1;
        const double gx = ((win[r][q + 2] - win[r][q]) + 2.0 * (win[r + 1][q + 2] - win[r + 1][q]) + (win[r + 2][q + 2] - win[r + 2][q])) / 8.0;
        const double gy = ((win[r + 2][q] - win[r][q]) + 2.0 * (win[r + 2][q + 1] - win[r][q + 1]) + (win[r + 2][q + 2] - win[r][q + 2])) / 8.0;
        sx[c] = s.in[c] ? gx : 0.0;
        sy[c] = s.in[c] ? gy : 0.0;
    }
}

// bilinear value of four corner values, and its derivatives with respect to the sample coordinate
__device__ __forceinline__ double bilinear(const Sample &s, const double *v) {
    return ((s.w[0] * v[0] + s.w[1] * v[1]) + s.w[2] * v[2]) + s.w[3] * v[3];
}
__device__ __forceinline__ double bilinear_dx(const Sample &s, const double *v) {
    return (1.0 - s.ty) * (v[1] - v[0]) + s.ty * (v[3] - v[2]);
}
__device__ __forceinline__ double bilinear_dy(const Sample &s, const double *v) {
    return (1.0 - s.tx) * (v[2] - v[0]) + s.tx * (v[3] - v[1]);
}

// the flow mask of generative_model: the channel sum of inp_cnt, 1 where it is positive and the sum itself elsewhere
__device__ __forceinline__ float flow_mask(const float *__restrict__ cnt, int C, int64_t b, int64_t pix, int64_t P) {
    float s = 0.f;
    for (int c = 0; c < C; ++c) s = s + cnt[(b * C + c) * P + pix];
    return s > 0.f ? 1.f : s;
}

struct Pixel {
    int64_t b, pix;
    int h, w;
};
__device__ __forceinline__ Pixel pixel_of(int64_t i, int H, int W) {
    const int64_t P = (int64_t)H * W;
    Pixel p;
    p.b = i / P, p.pix = i % P;
    p.h = (int)(p.pix / W), p.w = (int)(p.pix % W);
    return p;
}

// key and addends of the four scatter entries of source pixel i; g[plane] is d loss / d (sampled value) of that plane
template <int PLANES>
__device__ __forceinline__ void scatter_entries(const Sample &s, int64_t i, int64_t b, int64_t K, int H, int W, const double *g,
                                                uint32_t *__restrict__ keys, float *__restrict__ val) {
    const int64_t P = (int64_t)H * W, n = 4 * K;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const int64_t e = 4 * i + c;
        const int64_t dst = b * P + (int64_t)(s.y0 + (c >> 1)) * W + (s.x0 + (c & 1));
        keys[e] = s.in[c] ? (uint32_t)dst : (uint32_t)K;
#pragma unroll
        for (int p = 0; p < PLANES; ++p) val[(int64_t)p * n + e] = s.in[c] ? (float)(g[p] * s.w[c]) : 0.f;
    }
}

// ------------------------------------------------------------------ masked flow (what AveragedIWE reads)
__global__ void mask_flow(Flow4 flow, const float *__restrict__ cnt, int C, int64_t K, int H, int W, float *__restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= K) return;
    const Pixel p = pixel_of(i, H, W);
    const int64_t P = (int64_t)H * W;
    const float m = flow_mask(cnt, C, p.b, p.pix, P);
    const float *f = flow.p + p.b * flow.sb + p.h * flow.sh + p.w * flow.sw;
    out[(p.b * 2) * P + p.pix] = f[0] * m;
    out[(p.b * 2 + 1) * P + p.pix] = f[flow.sc] * m;
}

// ------------------------------------------------------------------ the generative-model term
// resid[i] = (avg+ - avg-) + (Sx * fx + Sy * fy) * S with the masked flow; partial sums of resid^2
__global__ void generative_forward(Flow4 flow, const float *__restrict__ img, const float *__restrict__ cnt, int C,
                                   const float *__restrict__ avg, int64_t K, int H, int W, double S, float *__restrict__ resid,
                                   double *__restrict__ partials) {
    __shared__ double buf[kBlock];
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    double v = 0.0;
    if (i < K) {
        const Pixel p = pixel_of(i, H, W);
        const int64_t P = (int64_t)H * W;
        const float m = flow_mask(cnt, C, p.b, p.pix, P);
        const float *f = flow.p + p.b * flow.sb + p.h * flow.sh + p.w * flow.sw;
        const float fx = f[0] * m, fy = f[flow.sc] * m;
        const Sample s = sample_at(p.h, p.w, fx, fy, S, H, W);
        double pred = 0.0;
        if (s.ok) {
            double sx[4], sy[4];
            corner_sobel(img + p.b * P, s, H, W, sx, sy);
            pred = (bilinear(s, sx) * (double)fx + bilinear(s, sy) * (double)fy) * S;
        }
        const double ev = (double)avg[(p.b * 2) * P + p.pix] - (double)avg[(p.b * 2 + 1) * P + p.pix];
        const float r = (float)(ev + pred);
        resid[i] = r;
        v = (double)r * (double)r;
    }
    const double total = block_sum(v, buf);
    if (threadIdx.x == 0) partials[blockIdx.x] = total;
}

// grad_flow [B, 2, H, W] contiguous (every element written once); keys / val: the scatter entries into the two Sobel
// gradient images (skipped when keys is null)
__global__ void generative_backward(Flow4 flow, const float *__restrict__ img, const float *__restrict__ cnt, int C,
                                    const float *__restrict__ resid, int64_t K, int H, int W, double S,
                                    const float *__restrict__ grad_out, float *__restrict__ grad_flow,
                                    uint32_t *__restrict__ keys, float *__restrict__ val) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= K) return;
    const Pixel p = pixel_of(i, H, W);
    const int64_t P = (int64_t)H * W;
    const float m = flow_mask(cnt, C, p.b, p.pix, P);
    const float *f = flow.p + p.b * flow.sb + p.h * flow.sh + p.w * flow.sw;
    const float fx = f[0] * m, fy = f[flow.sc] * m;
    const Sample s = sample_at(p.h, p.w, fx, fy, S, H, W);
    const double gp = 2.0 * (double)resid[i] * (double)grad_out[0] * S;      // d loss / d (Sx fx + Sy fy)
    double gx = 0.0, gy = 0.0;
    double g[2] = {gp * (double)fx, gp * (double)fy};                        // d loss / d (sampled Sx, sampled Sy)
    if (s.ok) {
        double sx[4], sy[4];
        corner_sobel(img + p.b * P, s, H, W, sx, sy);
        const double dix = -S * (double)W / (double)(W - 1), diy = -S * (double)H / (double)(H - 1);
        gx = gp * bilinear(s, sx) + (g[0] * bilinear_dx(s, sx) + g[1] * bilinear_dx(s, sy)) * dix;
        gy = gp * bilinear(s, sy) + (g[0] * bilinear_dy(s, sx) + g[1] * bilinear_dy(s, sy)) * diy;
    }
    if (grad_flow) {      // times the mask; a masked pixel gets +0
        grad_flow[(p.b * 2) * P + p.pix] = m == 0.f ? 0.f : (float)((double)m * gx);
        grad_flow[(p.b * 2 + 1) * P + p.pix] = m == 0.f ? 0.f : (float)((double)m * gy);
    }
    if (keys) scatter_entries<2>(s, i, p.b, K, H, W, g, keys, val);
}

// ------------------------------------------------------------------ Sobel
__global__ void sobel_forward(const float *__restrict__ x, int64_t K, int H, int W, float *__restrict__ gradx,
                              float *__restrict__ grady) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= K) return;
    const Pixel p = pixel_of(i, H, W);
    const float *plane = x + p.b * (int64_t)H * W;
    double win[3][3];
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int c = 0; c < 3; ++c) win[a][c] = (double)plane[(int64_t)clampi(p.h - 1 + a, H) * W + clampi(p.w - 1 + c, W)];
    gradx[i] = (float)(((win[0][2] - win[0][0]) + 2.0 * (win[1][2] - win[1][0]) + (win[2][2] - win[2][0])) / 8.0);
    grady[i] = (float)(((win[2][0] - win[0][0]) + 2.0 * (win[2][1] - win[0][1]) + (win[2][2] - win[0][2])) / 8.0);
}

// The adjoint with its replication pad, as a gather: pixel (h, w) collects, from every output pixel q within one step and every
// tap d of q whose clamped position is (h, w), tap_x(d) * ggx[q] + tap_y(d) * ggy[q], in a fixed order, float64, then / 8.
// ggx or ggy may be null (an output that drew no gradient).
__global__ void sobel_backward(const float *__restrict__ ggx, const float *__restrict__ ggy, int64_t K, int H, int W,
                               float *__restrict__ grad_x) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= K) return;
    const Pixel p = pixel_of(i, H, W);
    const int64_t base = p.b * (int64_t)H * W;
    double acc = 0.0;
    for (int qy = p.h - 1; qy <= p.h + 1; ++qy) {
        if (qy < 0 || qy >= H) continue;
        for (int qx = p.w - 1; qx <= p.w + 1; ++qx) {
            if (qx < 0 || qx >= W) continue;
            double ca = 0.0, cb = 0.0;      // the summed taps of q that land on (h, w): small integers, exact
            for (int dy = -1; dy <= 1; ++dy) {
                if (clampi(qy + dy, H) != p.h) continue;
                for (int dx = -1; dx <= 1; ++dx) {
                    if (clampi(qx + dx, W) != p.w) continue;
                    ca += (double)(dx * (dy == 0 ? 2 : 1));
                    cb += (double)(dy * (dx == 0 ? 2 : 1));
                }
            }
            const int64_t q = base + (int64_t)qy * W + qx;
            if (ggx) acc = acc + ca * (double)ggx[q];
            if (ggy) acc = acc + cb * (double)ggy[q];
        }
    }
    grad_x[i] = (float)(acc / 8.0);
}

// ------------------------------------------------------------------ the temporal-consistency term
// resid[i] = img - sample(prev_img) under the unmasked flow; partial sums of |resid|
__global__ void temporal_forward(Flow4 flow, const float *__restrict__ prev, const float *__restrict__ img, int64_t K, int H, int W,
                                 double S, float *__restrict__ resid, double *__restrict__ partials) {
    __shared__ double buf[kBlock];
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    double v = 0.0;
    if (i < K) {
        const Pixel p = pixel_of(i, H, W);
        const int64_t P = (int64_t)H * W;
        const float *f = flow.p + p.b * flow.sb + p.h * flow.sh + p.w * flow.sw;
        const Sample s = sample_at(p.h, p.w, f[0], f[flow.sc], S, H, W);
        double c[4];
#pragma unroll
        for (int k = 0; k < 4; ++k)
            c[k] = s.in[k] ? (double)prev[p.b * P + (int64_t)(s.y0 + (k >> 1)) * W + (s.x0 + (k & 1))] : 0.0;
        const float r = (float)((double)img[i] - bilinear(s, c));
        resid[i] = r;
        v = fabs((double)r);
    }
    const double total = block_sum(v, buf);
    if (threadIdx.x == 0) partials[blockIdx.x] = total;
}

__device__ __forceinline__ double sign_of(float v) { return v > 0.f ? 1.0 : (v < 0.f ? -1.0 : 0.0); }      // 0 at 0, NaN -> 0

__global__ void temporal_backward(Flow4 flow, const float *__restrict__ prev, const float *__restrict__ resid, int64_t K, int H,
                                  int W, double S, double weight, const float *__restrict__ grad_out,
                                  float *__restrict__ grad_flow, float *__restrict__ grad_img, uint32_t *__restrict__ keys,
                                  float *__restrict__ val) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= K) return;
    const Pixel p = pixel_of(i, H, W);
    const int64_t P = (int64_t)H * W;
    const float *f = flow.p + p.b * flow.sb + p.h * flow.sh + p.w * flow.sw;
    const Sample s = sample_at(p.h, p.w, f[0], f[flow.sc], S, H, W);
    const double gr = weight * (double)grad_out[0] * sign_of(resid[i]);      // d loss / d resid
    if (grad_img) grad_img[i] = (float)gr;
    const double g[1] = {-gr};                                               // d loss / d (sampled prev_img)
    if (grad_flow) {
        double c[4];
#pragma unroll
        for (int k = 0; k < 4; ++k)
            c[k] = s.in[k] ? (double)prev[p.b * P + (int64_t)(s.y0 + (k >> 1)) * W + (s.x0 + (k & 1))] : 0.0;
        const double dix = -S * (double)W / (double)(W - 1), diy = -S * (double)H / (double)(H - 1);
        grad_flow[(p.b * 2) * P + p.pix] = s.ok ? (float)(g[0] * bilinear_dx(s, c) * dix) : 0.f;
        grad_flow[(p.b * 2 + 1) * P + p.pix] = s.ok ? (float)(g[0] * bilinear_dy(s, c) * diy) : 0.f;
    }
    if (keys) scatter_entries<1>(s, i, p.b, K, H, W, g, keys, val);
}

// ------------------------------------------------------------------ total variation
__global__ void tv_forward(const float *__restrict__ img, int64_t K, int H, int W, double *__restrict__ partials) {
    __shared__ double buf[kBlock];
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    double v = 0.0;
    if (i < K) {
        const Pixel p = pixel_of(i, H, W);
        if (p.h + 1 < H) v = v + fabs((double)(img[i] - img[i + W]));
        if (p.w + 1 < W) v = v + fabs((double)(img[i] - img[i + 1]));
    }
    const double total = block_sum(v, buf);
    if (threadIdx.x == 0) partials[blockIdx.x] = total;
}

__global__ void tv_backward(const float *__restrict__ img, int64_t K, int H, int W, double weight, const float *__restrict__ grad_out,
                            float *__restrict__ grad_img) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= K) return;
    const Pixel p = pixel_of(i, H, W);
    double g = 0.0;
    if (p.h + 1 < H) g = g + sign_of(img[i] - img[i + W]);
    if (p.h > 0) g = g - sign_of(img[i - W] - img[i]);
    if (p.w + 1 < W) g = g + sign_of(img[i] - img[i + 1]);
    if (p.w > 0) g = g - sign_of(img[i - 1] - img[i]);
    grad_img[i] = (float)(weight * (double)grad_out[0] * g);
}

// ------------------------------------------------------------------ host side
constexpr size_t kAlign = 256;
inline size_t up(size_t v) { return (v + kAlign - 1) / kAlign * kAlign; }

constexpr int64_t kMaxEntries = ((int64_t)1 << 32) - 1;      // 4 * B * H * W: permutation entries and table sums are uint32
constexpr int64_t kMaxPixels = ((int64_t)1 << 32) - 2;       // B * H * W where nothing is sorted (Sobel, total variation)

struct Sort {
    uint32_t *keys[2], *perm[2], *hist, *sums;
    int64_t nb, m, nt;
};

// the partial sums stand first: a forward call needs no more than them
struct Layout {
    size_t partials, keys[2], perm[2], hist, sums, seg, val, gsob, forward, total;
    int64_t nb, m, nt, npart;
};

Layout layout(int64_t K) {
    Layout L;
    const int64_t n = 4 * K;
    L.nb = ceil_div(n, kBlock);
    L.m = 256 * L.nb;
    L.nt = ceil_div(L.m, kScanTile);
    L.npart = ceil_div(K, kBlock);
    size_t at = 0;
    auto take = [&at](size_t bytes) {
        const size_t here = at;
        at += up(bytes);
        return here;
    };
    L.partials = take((size_t)L.npart * 8);
    L.forward = at;
    for (int k = 0; k < 2; ++k) L.keys[k] = take((size_t)n * 4);
    for (int k = 0; k < 2; ++k) L.perm[k] = take((size_t)n * 4);
    L.hist = take((size_t)L.m * 4);
    L.sums = take((size_t)L.nt * 4);
    L.seg = take((size_t)(K + 2) * 4);
    L.val = take((size_t)n * 8);           // two planes of addends
    L.gsob = take((size_t)K * 8);          // the two Sobel gradient images
    L.total = at;
    return L;
}

template <typename T>
T *at(void *ws, size_t off) {
    return reinterpret_cast<T *>(static_cast<char *>(ws) + off);
}

#define BC_LAUNCH(label, kern, grid, ...)                                                 \
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

// Sorts n entries (n >= 1) whose keys lie in [0, maxkey] and stand in S.keys[0]; *cur names the result.
int radix_sort(Sort &S, int64_t n, int64_t maxkey, int *cur, hipStream_t st) {
    S.nb = ceil_div(n, kBlock);
    S.m = 256 * S.nb;
    S.nt = ceil_div(S.m, kScanTile);
    const int passes = key_passes(maxkey);
    for (int p = 0; p < passes; ++p) {
        const int shift = 8 * p, c = *cur;
        BC_LAUNCH("bc_sort_hist", sort_hist, dim3((unsigned)S.nb), S.keys[c], n, shift, S.hist, (int)S.nb);
        BC_LAUNCH("bc_scan_tiles", scan_tiles, dim3((unsigned)S.nt), S.hist, S.m, S.sums);
        BC_LAUNCH("bc_scan_sums", scan_sums, dim3(1), S.sums, S.nt);
        BC_LAUNCH("bc_sort_scatter", sort_scatter, dim3((unsigned)S.nb), S.keys[c], p == 0 ? (const uint32_t *)nullptr : S.perm[c], n,
                  shift, S.hist, S.sums, (int)S.nb, S.keys[c ^ 1], S.perm[c ^ 1]);
        *cur = c ^ 1;
    }
    return EBFI_OK;
}

// the entries in the workspace (keys[0], val) -> out [planes][K]: the ordered sum per destination pixel
int ordered_scatter(void *ws, const Layout &L, int64_t K, int planes, float *out, hipStream_t st) {
    Sort S;
    for (int k = 0; k < 2; ++k) S.keys[k] = at<uint32_t>(ws, L.keys[k]), S.perm[k] = at<uint32_t>(ws, L.perm[k]);
    S.hist = at<uint32_t>(ws, L.hist), S.sums = at<uint32_t>(ws, L.sums);
    const int64_t n = 4 * K;
    int cur = 0;
    if (int rc = radix_sort(S, n, K, &cur, st)) return rc;
    uint32_t *seg = at<uint32_t>(ws, L.seg);
    BC_LAUNCH("bc_run_starts", run_starts, dim3((unsigned)ceil_div(K + 1, kBlock)), S.keys[cur], n, K, seg);
    const dim3 grid((unsigned)ceil_div(K, kBlock));
    const float *val = at<float>(ws, L.val);
    if (planes == 1) {
        BC_LAUNCH("bc_accumulate", accumulate<1>, grid, val, n, S.perm[cur], seg, K, out);
    } else {
        BC_LAUNCH("bc_accumulate", accumulate<2>, grid, val, n, S.perm[cur], seg, K, out);
    }
    return EBFI_OK;
}

bool sizes_bad(int64_t B, int H, int W) { return B < 1 || H < 2 || W < 2; }
// sorts: the two sampling terms, whose backward sorts four entries per pixel; Sobel and the total variation index with int64
bool sizes_big(int64_t B, int H, int W, bool sorts) { return (int64_t)H * W > (sorts ? kMaxEntries / 4 : kMaxPixels) / B; }

int sizes_ok(const char *what, int64_t B, int H, int W, bool sorts = true) {
    if (sizes_bad(B, H, W)) return fail(EBFI_ERR_ARG, "%s: bad sizes (B >= 1, H >= 2 and W >= 2 are required)", what);
    if (sizes_big(B, H, W, sorts))
        return fail(EBFI_ERR_UNSUPPORTED, sorts ? "%s: 4 * B * H * W >= 2^32" : "%s: B * H * W >= 2^32 - 1", what);
    return EBFI_OK;
}

int workspace_ok(const char *what, size_t need, const void *ws, int64_t bytes) {
    if (!ws || bytes < (int64_t)need) return fail(EBFI_ERR_WORKSPACE, "%s: workspace too small", what);
    if (!aligned16(ws)) return fail(EBFI_ERR_ARG, "%s: workspace not 16-byte aligned", what);
    return EBFI_OK;
}

}  // namespace

extern "C" int64_t ebfi_bc_workspace(int64_t B, int H, int W) {
    if (sizes_bad(B, H, W) || sizes_big(B, H, W, true)) return 0;
    return (int64_t)layout(B * (int64_t)H * W).total;
}

extern "C" int64_t ebfi_bc_forward_workspace(int64_t B, int H, int W) {
    if (sizes_bad(B, H, W) || sizes_big(B, H, W, false)) return 0;      // (the partial sums only: the total variation too)
    return (int64_t)layout(B * (int64_t)H * W).forward;
}

extern "C" int ebfi_sobel_forward(const float *x, int64_t planes, int H, int W, float *gradx, float *grady, void *stream) {
    if (int rc = sizes_ok("sobel_forward", planes, H, W, false)) return rc;
    if (!x || !gradx || !grady) return fail(EBFI_ERR_ARG, "sobel_forward: null pointer");
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int64_t K = planes * (int64_t)H * W;
    BC_LAUNCH("sobel_forward", sobel_forward, dim3((unsigned)ceil_div(K, kBlock)), x, K, H, W, gradx, grady);
    return EBFI_OK;
}

extern "C" int ebfi_sobel_backward(const float *grad_gradx, const float *grad_grady, int64_t planes, int H, int W, float *grad_x,
                                   void *stream) {
    if (int rc = sizes_ok("sobel_backward", planes, H, W, false)) return rc;
    if ((!grad_gradx && !grad_grady) || !grad_x) return fail(EBFI_ERR_ARG, "sobel_backward: null pointer");
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int64_t K = planes * (int64_t)H * W;
    BC_LAUNCH("sobel_backward", sobel_backward, dim3((unsigned)ceil_div(K, kBlock)), grad_gradx, grad_grady, K, H, W, grad_x);
    return EBFI_OK;
}

extern "C" int ebfi_bc_mask_flow(const float *flow, int64_t flow_sb, int64_t flow_sc, int64_t flow_sh, int64_t flow_sw,
                                 const float *cnt, int C, int64_t B, int H, int W, float *masked, void *stream) {
    if (int rc = sizes_ok("bc_mask_flow", B, H, W)) return rc;
    if (C < 1) return fail(EBFI_ERR_ARG, "bc_mask_flow: inp_cnt needs at least one channel, got %d", C);
    if (!flow || !cnt || !masked) return fail(EBFI_ERR_ARG, "bc_mask_flow: null pointer");
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int64_t K = B * (int64_t)H * W;
    BC_LAUNCH("bc_mask_flow", mask_flow, dim3((unsigned)ceil_div(K, kBlock)), Flow4{flow, flow_sb, flow_sc, flow_sh, flow_sw}, cnt, C,
              K, H, W, masked);
    return EBFI_OK;
}

extern "C" int ebfi_bc_generative_forward(const float *flow, int64_t flow_sb, int64_t flow_sc, int64_t flow_sh, int64_t flow_sw,
                                          const float *img, const float *cnt, int C, const float *avg, int64_t B, int H, int W,
                                          float flow_scaling, float *resid, float *loss, void *workspace, int64_t workspace_bytes,
                                          void *stream) {
    if (int rc = sizes_ok("bc_generative_forward", B, H, W)) return rc;
    if (C < 1) return fail(EBFI_ERR_ARG, "bc_generative_forward: inp_cnt needs at least one channel, got %d", C);
    if (!flow || !img || !cnt || !avg || !resid || !loss) return fail(EBFI_ERR_ARG, "bc_generative_forward: null pointer");
    const int64_t K = B * (int64_t)H * W;
    const Layout L = layout(K);
    if (int rc = workspace_ok("bc_generative_forward", L.forward, workspace, workspace_bytes)) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    double *partials = at<double>(workspace, L.partials);
    BC_LAUNCH("bc_generative_forward", generative_forward, dim3((unsigned)L.npart), Flow4{flow, flow_sb, flow_sc, flow_sh, flow_sw}, img,
              cnt, C, avg, K, H, W, (double)flow_scaling, resid, partials);
    BC_LAUNCH("bc_loss_final", loss_final, dim3(1), partials, L.npart, 1.0, loss);
    return EBFI_OK;
}

extern "C" int ebfi_bc_generative_backward(const float *flow, int64_t flow_sb, int64_t flow_sc, int64_t flow_sh, int64_t flow_sw,
                                           const float *img, const float *cnt, int C, const float *resid, int64_t B, int H, int W,
                                           float flow_scaling, const float *grad_out, float *grad_flow, float *grad_img,
                                           void *workspace, int64_t workspace_bytes, void *stream) {
    if (int rc = sizes_ok("bc_generative_backward", B, H, W)) return rc;
    if (C < 1) return fail(EBFI_ERR_ARG, "bc_generative_backward: inp_cnt needs at least one channel, got %d", C);
    if (!flow || !img || !cnt || !resid || !grad_out || (!grad_flow && !grad_img))
        return fail(EBFI_ERR_ARG, "bc_generative_backward: null pointer");
    const int64_t K = B * (int64_t)H * W;
    const Layout L = layout(K);
    if (int rc = workspace_ok("bc_generative_backward", grad_img ? L.total : L.forward, workspace, workspace_bytes)) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)ceil_div(K, kBlock));
    BC_LAUNCH("bc_generative_backward", generative_backward, grid, Flow4{flow, flow_sb, flow_sc, flow_sh, flow_sw}, img, cnt, C, resid, K,
              H, W, (double)flow_scaling, grad_out, grad_flow, grad_img ? at<uint32_t>(workspace, L.keys[0]) : (uint32_t *)nullptr,
              at<float>(workspace, L.val));
    if (!grad_img) return EBFI_OK;
    float *gsob = at<float>(workspace, L.gsob);
    if (int rc = ordered_scatter(workspace, L, K, 2, gsob, st)) return rc;
    BC_LAUNCH("sobel_backward", sobel_backward, grid, gsob, gsob + K, K, H, W, grad_img);
    return EBFI_OK;
}

extern "C" int ebfi_bc_temporal_forward(const float *flow, int64_t flow_sb, int64_t flow_sc, int64_t flow_sh, int64_t flow_sw,
                                        const float *prev_img, const float *img, int64_t B, int H, int W, float flow_scaling,
                                        double weight, float *resid, float *loss, void *workspace, int64_t workspace_bytes,
                                        void *stream) {
    if (int rc = sizes_ok("bc_temporal_forward", B, H, W)) return rc;
    if (!flow || !prev_img || !img || !resid || !loss) return fail(EBFI_ERR_ARG, "bc_temporal_forward: null pointer");
    const int64_t K = B * (int64_t)H * W;
    const Layout L = layout(K);
    if (int rc = workspace_ok("bc_temporal_forward", L.forward, workspace, workspace_bytes)) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    double *partials = at<double>(workspace, L.partials);
    BC_LAUNCH("bc_temporal_forward", temporal_forward, dim3((unsigned)L.npart), Flow4{flow, flow_sb, flow_sc, flow_sh, flow_sw}, prev_img,
              img, K, H, W, (double)flow_scaling, resid, partials);
    BC_LAUNCH("bc_loss_final", loss_final, dim3(1), partials, L.npart, weight, loss);
    return EBFI_OK;
}

extern "C" int ebfi_bc_temporal_backward(const float *flow, int64_t flow_sb, int64_t flow_sc, int64_t flow_sh, int64_t flow_sw,
                                         const float *prev_img, const float *resid, int64_t B, int H, int W, float flow_scaling,
                                         double weight, const float *grad_out, float *grad_flow, float *grad_prev, float *grad_img,
                                         void *workspace, int64_t workspace_bytes, void *stream) {
    if (int rc = sizes_ok("bc_temporal_backward", B, H, W)) return rc;
    if (!flow || !prev_img || !resid || !grad_out || (!grad_flow && !grad_prev && !grad_img))
        return fail(EBFI_ERR_ARG, "bc_temporal_backward: null pointer");
    const int64_t K = B * (int64_t)H * W;
    const Layout L = layout(K);
    if (int rc = workspace_ok("bc_temporal_backward", grad_prev ? L.total : L.forward, workspace, workspace_bytes)) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    BC_LAUNCH("bc_temporal_backward", temporal_backward, dim3((unsigned)ceil_div(K, kBlock)),
              Flow4{flow, flow_sb, flow_sc, flow_sh, flow_sw}, prev_img, resid, K, H, W, (double)flow_scaling, weight, grad_out, grad_flow,
              grad_img, grad_prev ? at<uint32_t>(workspace, L.keys[0]) : (uint32_t *)nullptr, at<float>(workspace, L.val));
    if (!grad_prev) return EBFI_OK;
    return ordered_scatter(workspace, L, K, 1, grad_prev, st);
}

extern "C" int ebfi_bc_tv_forward(const float *img, int64_t planes, int H, int W, double weight, float *loss, void *workspace,
                                  int64_t workspace_bytes, void *stream) {
    if (int rc = sizes_ok("bc_tv_forward", planes, H, W, false)) return rc;
    if (!img || !loss) return fail(EBFI_ERR_ARG, "bc_tv_forward: null pointer");
    const int64_t K = planes * (int64_t)H * W;
    const Layout L = layout(K);
    if (int rc = workspace_ok("bc_tv_forward", L.forward, workspace, workspace_bytes)) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    double *partials = at<double>(workspace, L.partials);
    BC_LAUNCH("bc_tv_forward", tv_forward, dim3((unsigned)L.npart), img, K, H, W, partials);
    BC_LAUNCH("bc_loss_final", loss_final, dim3(1), partials, L.npart, weight, loss);
    return EBFI_OK;
}

extern "C" int ebfi_bc_tv_backward(const float *img, int64_t planes, int H, int W, double weight, const float *grad_out,
                                   float *grad_img, void *stream) {
    if (int rc = sizes_ok("bc_tv_backward", planes, H, W, false)) return rc;
    if (!img || !grad_out || !grad_img) return fail(EBFI_ERR_ARG, "bc_tv_backward: null pointer");
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int64_t K = planes * (int64_t)H * W;
    BC_LAUNCH("bc_tv_backward", tv_backward, dim3((unsigned)ceil_div(K, kBlock)), img, K, H, W, weight, grad_out, grad_img);
    return EBFI_OK;
}
