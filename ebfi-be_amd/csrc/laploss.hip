// Laplacian-pyramid L1 loss of the training step as one pyramid of the DIFFERENCE image.
//
// Reference: loss/restore.py:149-213 (GaussianConv 5x5 reflect, LaplacianPyramid with avg_pool2d reduce and
// zero-insertion expand x4, LaplacianLoss = sum_i 2^i * L1sum(lap_i(x), lap_i(y))), applied to two predictions
// against the same target in train_ours.py:258-268.  Every pyramid operator is linear, so
// lap_i(x) - lap_i(y) = lap_i(x - y): ONE pyramid over the planes [a - t ; b - t] replaces the three pyramids of a
// step, and each level is two kernels (reduce; expand + subtract + |.| + partial sums) instead of ~15 elementwise
// passes.
//
// Kernels (all: one workgroup of 256 threads per plane tile, the tile's input staged once in LDS with coalesced loads):
//   lap_reduce<DIFF>  16x16 outputs from a 36x36 tile (halo 2, reflection resolved while staging); a thread blurs its 6x6
//                     window from LDS (8-byte reads) and pools the 2x2 cell.  DIFF (level 0) forms a - t / b - t while
//                     staging and writes cur_0: there is no separate difference pass.
//   lap_level         32x32 outputs, a thread owns a 2x2 cell: the zero-inserted image has a value only at even
//                     positions, so the cell's four pixels use 9 / 6 / 6 / 4 fixed taps of the 3x3 coarse
//                     neighbourhood (18x18 tile of `red`), no per-tap test.
//   lap_bwd_reduce    16x16 outputs from a 36x36 tile of s; pixels >= 3 away from every edge take 25 fixed taps from
//                     LDS, the frame takes the general adjoint (mirror images of the reflect padding), also from LDS.
//   lap_bwd_expand    32x32 outputs, a thread owns a 2x2 cell and the 3x3 neighbourhood of g / 4 (18x18 tile): six
//                     horizontal sums serve the four pixels; cells within 4 of an edge take the general adjoint.
//   lap_last          coarsest level (no expand): elementwise.
// The general adjoint (gauss5_adj) has no loop over mirror images and no dependent loads: it sums each of the five
// candidate source rows once and runs the vertical chain over those sums (what paced the one-thread-per-pixel
// kernels was its chain of 25-225 load-then-use iterations, profiles/loss_pack/README.md).
//
// Arithmetic: the value of every pixel is computed by the same operations in the same order as the one-thread-per-pixel
// kernels this file started with (taps a zero-inserted or out-of-image position would contribute are skipped, as they
// were).  Contraction is switched off for the file and every fused multiply-add is written out, so the rounding does
// not depend on how the compiler schedules a kernel: the blur and both adjoints accumulate with fma throughout (as
// gauss5_fwd / gauss5_bwd of imgops.hip do), the expand of lap_level accumulates its horizontal sums with fma and adds
// the rounded products k[i] * hsum of its rows.  Only the order in which per-workgroup partial sums are added depends
// on the tiling.
//
// Workspace (floats): level images cur_0 .. cur_{L-1}, level l at offset sum_{k<l} planes*H*W/4^k.  Forward
// overwrites cur_l with s_l = coef(plane) * 2^l * sign(lap_l) (what the backward needs); backward consumes the
// workspace in place (g_{l+1} -= 4 G^T(s_l) at even positions; s_l += G^T(P^T g_{l+1})) -> it can run once per forward.
#include "common.hpp"

#pragma clang fp contract(off)

using namespace ebfi;

namespace {

constexpr int LT = 256;
constexpr int RT = 16;            // reduce kernels: output tile edge (one thread per output)
constexpr int RI = 2 * RT + 4;    //                 staged input tile edge (even: 8-byte LDS reads)
constexpr int ET = 32;            // level / expand kernels: output tile edge (one thread per 2x2 cell)
constexpr int EC = ET / 2 + 2;    //                 staged coarse tile edge
constexpr int RN = (RI * RI + LT - 1) / LT, EN = (EC * EC + LT - 1) / LT;   // staging rounds of a workgroup
constexpr float K0 = 1.f / 16, K1 = 4.f / 16, K2 = 6.f / 16;   // the blur taps {K0, K1, K2, K1, K0}

__device__ __forceinline__ int reflect_idx(int i, int n) {
    if (i < 0) return -i;
    if (i >= n) return 2 * (n - 1) - i;
    return i;
}

struct Coef {
    float c[2];
    int64_t planes_per_term;
};

__device__ __forceinline__ float block_sum(float v, float *red) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) red[wave] = v;
    __syncthreads();
    float s = 0.f;
    if (threadIdx.x == 0)
        for (int w = 0; w < LT / 64; ++w) s += red[w];
    return s;
}

// blockIdx.x -> (plane, tile row, tile column)
__device__ __forceinline__ void tile_of(int tiles_y, int tiles_x, int64_t &p, int &ty, int &tx) {
    const unsigned per = (unsigned)tiles_y * (unsigned)tiles_x, pl = blockIdx.x / per;
    p = pl;
    const int r = (int)(blockIdx.x - pl * per);
    ty = r / tiles_x;
    tx = r - ty * tiles_x;
}

__device__ __forceinline__ float blur5(float v0, float v1, float v2, float v3, float v4) {
    float a = __builtin_fmaf(K0, v0, 0.f);
    a = __builtin_fmaf(K1, v1, a);
    a = __builtin_fmaf(K2, v2, a);
    a = __builtin_fmaf(K1, v3, a);
    return __builtin_fmaf(K0, v4, a);
}

// red = avg_pool2d(gauss5(cur), 2): the four blurred values of a 2x2 cell from one 6x6 window.
// DIFF: cur = [a - t ; b - t] is formed while staging and written out as cur_0 (b may be null: one term).
template <bool DIFF>
__global__ __launch_bounds__(LT) void lap_reduce_kernel(const float *__restrict__ src, const float *__restrict__ a,
                                                        const float *__restrict__ b, const float *__restrict__ t,
                                                        float *__restrict__ cur, float *__restrict__ red, int64_t ppt, int H,
                                                        int W, int tiles_y, int tiles_x) {
    __shared__ __attribute__((aligned(8))) float tile[RI][RI];
    int64_t p;
    int ty, tx;
    tile_of(tiles_y, tiles_x, p, ty, tx);
    const int64_t hw = (int64_t)H * W;
    const int Y0 = 2 * RT * ty - 2, X0 = 2 * RT * tx - 2;
    const float *pa = nullptr, *pt = nullptr;
    if constexpr (DIFF) {
        const bool second = p >= ppt;
        pa = second ? b + (p - ppt) * hw : a + p * hw;
        pt = t + (second ? p - ppt : p) * hw;
    } else {
        pa = src + p * hw;
    }
    // all loads of a thread are issued before the first is used: positions a ragged tile does not need are clamped
    // into the image (loaded, never read back)
    float v[RN], vt[RN];
#pragma unroll
    for (int k = 0; k < RN; ++k) {
        const int i = threadIdx.x + k * LT, ly = i / RI, lx = i - ly * RI;
        const int gy = reflect_idx(min(Y0 + ly, H + 1), H), gx = reflect_idx(min(X0 + lx, W + 1), W);   // Y0, X0 >= -2
        const int64_t o = (int64_t)gy * W + gx;
        v[k] = pa[o];
        if constexpr (DIFF) vt[k] = pt[o];
    }
#pragma unroll
    for (int k = 0; k < RN; ++k) {
        const int i = threadIdx.x + k * LT, ly = i / RI, lx = i - ly * RI;
        if (i >= RI * RI) break;
        if constexpr (DIFF) {
            v[k] = v[k] - vt[k];
            const int vy = Y0 + ly, vx = X0 + lx;
            if (ly >= 2 && ly < RI - 2 && lx >= 2 && lx < RI - 2 && vy < H && vx < W) cur[p * hw + (int64_t)vy * W + vx] = v[k];
        }
        tile[ly][lx] = v[k];
    }
    __syncthreads();
    const int h = H >> 1, w = W >> 1;
    const int ry = threadIdx.x / RT, rx = threadIdx.x % RT;
    const int y = RT * ty + ry, x = RT * tx + rx;
    if (y >= h || x >= w) return;
    float h0[6], h1[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        const float2 *row = reinterpret_cast<const float2 *>(&tile[2 * ry + i][2 * rx]);
        const float2 v01 = row[0], v23 = row[1], v45 = row[2];
        h0[i] = blur5(v01.x, v01.y, v23.x, v23.y, v45.x);
        h1[i] = blur5(v01.y, v23.x, v23.y, v45.x, v45.y);
    }
    const float g00 = blur5(h0[0], h0[1], h0[2], h0[3], h0[4]);
    const float g01 = blur5(h1[0], h1[1], h1[2], h1[3], h1[4]);
    const float g10 = blur5(h0[1], h0[2], h0[3], h0[4], h0[5]);
    const float g11 = blur5(h1[1], h1[2], h1[3], h1[4], h1[5]);
    red[p * ((int64_t)h * w) + (int64_t)y * w + x] = (((g00 + g01) + g10) + g11) * 0.25f;
}

__device__ __forceinline__ float lap_finish(float lap, float cw, float &contrib) {
    contrib = cw * fabsf(lap);
    return lap > 0.f ? cw : (lap < 0.f ? -cw : 0.f);
}

// lap = cur - 4 * gauss5(zero_insert(red));  partial[block] = sum coef * weight * |lap|;  cur <- coef * weight * sign(lap)
// H, W even.  The zero-inserted image is non-zero at even positions only, and reflection keeps parity, so an even
// row (column) takes taps 0, 2, 4 of the coarse rows (columns) c-1, c, c+1 and an odd one taps 1, 3 of c, c+1.
__global__ __launch_bounds__(LT) void lap_level_kernel(float *__restrict__ cur, const float *__restrict__ red,
                                                       float *__restrict__ partial, int H, int W, int tiles_y, int tiles_x,
                                                       float weight, Coef cf) {
    __shared__ float r[EC][EC + 1];
    __shared__ float sred[LT / 64];
    int64_t p;
    int ty, tx;
    tile_of(tiles_y, tiles_x, p, ty, tx);
    const int h = H >> 1, w = W >> 1;
    const int64_t hw = (int64_t)H * W;
    const float *src = red + p * (hw >> 2);
    const int R0 = (ET / 2) * ty - 1, C0 = (ET / 2) * tx - 1;
    float v[EN];
#pragma unroll
    for (int k = 0; k < EN; ++k) {
        const int i = threadIdx.x + k * LT, ly = i / EC, lx = i - ly * EC;
        const int rv = min(R0 + ly, h), cv = min(C0 + lx, w);      // coarse position of the even pixel (2 rv, 2 cv), >= -1
        v[k] = src[(int64_t)(reflect_idx(2 * rv, H) >> 1) * w + (reflect_idx(2 * cv, W) >> 1)];
    }
#pragma unroll
    for (int k = 0; k < EN; ++k) {
        const int i = threadIdx.x + k * LT, ly = i / EC, lx = i - ly * EC;
        if (i < EC * EC) r[ly][lx] = v[k];
    }
    __syncthreads();
    const int cy = threadIdx.x / (ET / 2), cx = threadIdx.x % (ET / 2);
    const int y0 = ET * ty + 2 * cy, x0 = ET * tx + 2 * cx;
    float contrib = 0.f;
    if (y0 < H && x0 < W) {
        float he[3], ho[3];     // horizontal sums of the three coarse rows for an even / odd column
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const float q0 = r[cy + a][cx], q1 = r[cy + a][cx + 1], q2 = r[cy + a][cx + 2];
            he[a] = __builtin_fmaf(K0, q2, __builtin_fmaf(K2, q1, __builtin_fmaf(K0, q0, 0.f)));
            ho[a] = __builtin_fmaf(K1, q2, __builtin_fmaf(K1, q1, 0.f));
        }
        // rows: products rounded, then added (rows of the other parity add k * 0)
        const float e0 = ((K0 * he[0] + K1 * 0.f) + K2 * he[1]) + K1 * 0.f + K0 * he[2];
        const float e1 = ((K0 * ho[0] + K1 * 0.f) + K2 * ho[1]) + K1 * 0.f + K0 * ho[2];
        const float o0 = ((K0 * 0.f + K1 * he[1]) + K2 * 0.f) + K1 * he[2] + K0 * 0.f;
        const float o1 = ((K0 * 0.f + K1 * ho[1]) + K2 * 0.f) + K1 * ho[2] + K0 * 0.f;
        float *c0 = cur + p * hw + (int64_t)y0 * W + x0, *c1 = c0 + W;
        const float2 u0 = *reinterpret_cast<const float2 *>(c0), u1 = *reinterpret_cast<const float2 *>(c1);
        const float cw = cf.c[p >= cf.planes_per_term ? 1 : 0] * weight;
        float t00, t01, t10, t11;
        float2 s0, s1;
        s0.x = lap_finish(__builtin_fmaf(-4.f, e0, u0.x), cw, t00);
        s0.y = lap_finish(__builtin_fmaf(-4.f, e1, u0.y), cw, t01);
        s1.x = lap_finish(__builtin_fmaf(-4.f, o0, u1.x), cw, t10);
        s1.y = lap_finish(__builtin_fmaf(-4.f, o1, u1.y), cw, t11);
        *reinterpret_cast<float2 *>(c0) = s0;
        *reinterpret_cast<float2 *>(c1) = s1;
        contrib = ((t00 + t01) + t10) + t11;
    }
    const float s = block_sum(contrib, sred);
    if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

// coarsest level: lap = cur
__global__ __launch_bounds__(LT) void lap_last_kernel(float *__restrict__ cur, float *__restrict__ partial, int64_t n, int64_t hw,
                                                      float weight, Coef cf) {
    __shared__ float sred[LT / 64];
    const int64_t idx = (int64_t)blockIdx.x * LT + threadIdx.x;
    float contrib = 0.f;
    if (idx < n) {
        const float cw = cf.c[idx / hw >= cf.planes_per_term ? 1 : 0] * weight;
        cur[idx] = lap_finish(cur[idx], cw, contrib);
    }
    const float s = block_sum(contrib, sred);
    if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

// One axis of the adjoint of the reflect-padded blur at position p of n (n >= 4): u[c] is the term at p + 2 - c.  The
// padding maps up to three virtual positions onto p -- p itself, then -p (p = 1, 2), then 2 (n - 1) - p (p = n - 3,
// n - 2) -- and each contributes its taps j = 0..4 at o = virtual - j + 2 where 0 <= o < n: for p itself that is u[j];
// the mirror images reach back onto u[2], u[3] (p = 1), u[4] (p = 2), u[1], u[2] (p = n - 2), u[0] (p = n - 3).
__device__ __forceinline__ float adj_axis(const float (&u)[5], int p, int n) {
    const float k[5] = {K0, K1, K2, K1, K0};
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < 5; ++j) {
        const int o = p - j + 2;
        s = (o >= 0 && o < n) ? __builtin_fmaf(k[j], u[j], s) : s;
    }
    const bool lo1 = p == 1, lo2 = p == 2, hi1 = p == n - 2, hi2 = p == n - 3;
    s = lo1 ? __builtin_fmaf(K0, u[2], s) : (lo2 ? __builtin_fmaf(K0, u[4], s) : s);
    s = lo1 ? __builtin_fmaf(K1, u[3], s) : s;
    s = hi1 ? __builtin_fmaf(K1, u[1], s) : (hi2 ? __builtin_fmaf(K0, u[0], s) : s);
    s = hi1 ? __builtin_fmaf(K0, u[2], s) : s;
    return s;
}

// adjoint of the reflect-padded blur at (y, x), any pixel: sum over [virtual row][tap i][virtual column][tap j], terms
// outside the image skipped.  The horizontal sum of a source row does not depend on which (virtual row, tap) asks for
// it, so the five candidate rows y+2 .. y-2 are summed once each and the vertical chain picks from them.  Every term
// lies within 2 of (y, x): `at` is a lookup in the staged tile, called with positions clamped into the image (the
// clamped ones belong to skipped terms).
template <class F> __device__ __forceinline__ float gauss5_adj(int y, int x, int H, int W, F at) {
    int oxc[5];
#pragma unroll
    for (int c = 0; c < 5; ++c) oxc[c] = min(max(x + 2 - c, 0), W - 1);
    float hs[5];
#pragma unroll
    for (int r = 0; r < 5; ++r) {
        const int oyc = min(max(y + 2 - r, 0), H - 1);
        float u[5];
#pragma unroll
        for (int c = 0; c < 5; ++c) u[c] = at(oyc, oxc[c]);
        hs[r] = adj_axis(u, x, W);
    }
    return adj_axis(hs, y, H);
}

// g[y,x] (H/2 x W/2) += -4 * G^T(s)[2y, 2x]      (gradient reaching `red` through the expand path)
__global__ __launch_bounds__(LT) void lap_bwd_reduce_kernel(const float *__restrict__ s, float *__restrict__ g, int H, int W,
                                                            int tiles_y, int tiles_x) {
    __shared__ __attribute__((aligned(8))) float tile[RI][RI];
    int64_t p;
    int ty, tx;
    tile_of(tiles_y, tiles_x, p, ty, tx);
    const float *src = s + p * (int64_t)H * W;
    const int Y0 = 2 * RT * ty - 2, X0 = 2 * RT * tx - 2;
    float v[RN];     // (positions outside the image are clamped into it: loaded, never read back)
#pragma unroll
    for (int k = 0; k < RN; ++k) {
        const int i = threadIdx.x + k * LT, ly = i / RI, lx = i - ly * RI;
        v[k] = src[(int64_t)min(max(Y0 + ly, 0), H - 1) * W + min(max(X0 + lx, 0), W - 1)];
    }
#pragma unroll
    for (int k = 0; k < RN; ++k) {
        const int i = threadIdx.x + k * LT, ly = i / RI, lx = i - ly * RI;
        if (i < RI * RI) tile[ly][lx] = v[k];
    }
    __syncthreads();
    const int h = H >> 1, w = W >> 1;
    const int ry = threadIdx.x / RT, rx = threadIdx.x % RT;
    const int y = RT * ty + ry, x = RT * tx + rx;
    if (y >= h || x >= w) return;
    float adj;
    if (y >= 2 && y <= h - 2 && x >= 2 && x <= w - 2) {
        // (2y, 2x) is >= 3 away from every edge: rows 2y+2 .. 2y-2, columns 2x+2 .. 2x-2, nothing mirrored
        adj = 0.f;
        const float k[5] = {K0, K1, K2, K1, K0};
#pragma unroll
        for (int i = 0; i < 5; ++i) {
            const float2 *row = reinterpret_cast<const float2 *>(&tile[2 * ry + 4 - i][2 * rx]);
            const float2 v01 = row[0], v23 = row[1];
            const float v4 = tile[2 * ry + 4 - i][2 * rx + 4];
            adj = __builtin_fmaf(k[i], blur5(v4, v23.y, v23.x, v01.y, v01.x), adj);
        }
    } else {
        adj = gauss5_adj(2 * y, 2 * x, H, W, [&](int oy, int ox) { return tile[oy - Y0][ox - X0]; });
    }
    float *dst = g + p * ((int64_t)h * w) + (int64_t)y * w + x;
    *dst = __builtin_fmaf(-4.f, adj, *dst);
}

// out[y,x] = (s[y,x] + G^T(P^T g)[y,x]) * scale,  P^T g = g[y/2, x/2] / 4       (out may alias s)
__global__ __launch_bounds__(LT) void lap_bwd_expand_kernel(const float *s, const float *__restrict__ g, float *out,
                                                            const float *__restrict__ scale, int H, int W, int tiles_y,
                                                            int tiles_x) {
    __shared__ float q[EC][EC + 1];
    int64_t p;
    int ty, tx;
    tile_of(tiles_y, tiles_x, p, ty, tx);
    const int h = H >> 1, w = W >> 1;
    const int64_t hw = (int64_t)H * W;
    const float *src = g + p * (hw >> 2);
    const int R0 = (ET / 2) * ty - 1, C0 = (ET / 2) * tx - 1;
    float v[EN];
#pragma unroll
    for (int k = 0; k < EN; ++k) {
        const int i = threadIdx.x + k * LT, ly = i / EC, lx = i - ly * EC;
        v[k] = src[(int64_t)min(max(R0 + ly, 0), h - 1) * w + min(max(C0 + lx, 0), w - 1)];
    }
#pragma unroll
    for (int k = 0; k < EN; ++k) {
        const int i = threadIdx.x + k * LT, ly = i / EC, lx = i - ly * EC;
        if (i < EC * EC) q[ly][lx] = v[k] * 0.25f;
    }
    __syncthreads();
    const int cy = threadIdx.x / (ET / 2), cx = threadIdx.x % (ET / 2);
    const int gy = (ET / 2) * ty + cy, gx = (ET / 2) * tx + cx;     // the cell = the coarse pixel under it
    if (gy >= h || gx >= w) return;
    const int y0 = 2 * gy, x0 = 2 * gx;
    float adj[2][2];
    if (gy >= 2 && gy <= h - 3 && gx >= 2 && gx <= w - 3) {
        // all four pixels are >= 3 away from every edge.  Source rows of taps 0..4: c+1, c, c, c-1, c-1 for an even
        // row and c+1, c+1, c, c, c-1 for an odd one (columns alike): six horizontal sums serve the four pixels.
        float he[3], ho[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const float q0 = q[cy + a][cx], q1 = q[cy + a][cx + 1], q2 = q[cy + a][cx + 2];
            he[a] = blur5(q2, q1, q1, q0, q0);
            ho[a] = blur5(q2, q2, q1, q1, q0);
        }
        adj[0][0] = blur5(he[2], he[1], he[1], he[0], he[0]);
        adj[0][1] = blur5(ho[2], ho[1], ho[1], ho[0], ho[0]);
        adj[1][0] = blur5(he[2], he[2], he[1], he[1], he[0]);
        adj[1][1] = blur5(ho[2], ho[2], ho[1], ho[1], ho[0]);
    } else {
#pragma unroll
        for (int dy = 0; dy < 2; ++dy)
#pragma unroll
            for (int dx = 0; dx < 2; ++dx)
                adj[dy][dx] = gauss5_adj(y0 + dy, x0 + dx, H, W,
                                         [&](int oy, int ox) { return q[(oy >> 1) - R0][(ox >> 1) - C0]; });
    }
    const int64_t o = p * hw + (int64_t)y0 * W + x0;
    const float2 u0 = *reinterpret_cast<const float2 *>(s + o), u1 = *reinterpret_cast<const float2 *>(s + o + W);
    float2 v0, v1;
    v0.x = u0.x + adj[0][0];
    v0.y = u0.y + adj[0][1];
    v1.x = u1.x + adj[1][0];
    v1.y = u1.y + adj[1][1];
    if (scale) {
        const float sc = scale[0];
        v0.x *= sc;
        v0.y *= sc;
        v1.x *= sc;
        v1.y *= sc;
    }
    *reinterpret_cast<float2 *>(out + o) = v0;
    *reinterpret_cast<float2 *>(out + o + W) = v1;
}

bool lap_dims_ok(int64_t planes_per_term, int H, int W, int levels) {
    if (planes_per_term <= 0 || levels < 2 || levels > 8 || H < 3 || W < 3) return false;
    const int m = 1 << (levels - 1);
    if (H % m || W % m) return false;
    return H / (m / 2) >= 3 && W / (m / 2) >= 3;   // the coarsest blurred level still reflects
}

// workgroups of a tiled launch over `planes` images of h x w outputs in tiles of edge `tile`
int64_t tiles(int n, int tile) { return ceil_div(n, tile); }
int64_t tiled_blocks(int64_t planes, int h, int w, int tile) { return planes * tiles(h, tile) * tiles(w, tile); }

int64_t level_partials(int64_t planes, int H, int W, int levels, int l) {
    const int h = H >> l, w = W >> l;
    return l + 1 < levels ? tiled_blocks(planes, h, w, ET) : ceil_div(planes * (int64_t)h * w, LT);
}

}  // namespace

extern "C" int64_t ebfi_laploss_workspace_floats(int64_t planes, int H, int W, int levels) {
    int64_t n = 0;
    for (int l = 0; l < levels; ++l) n += planes * (int64_t)(H >> l) * (W >> l);
    return n;
}

extern "C" int64_t ebfi_laploss_partials(int64_t planes, int H, int W, int levels) {
    int64_t n = 0;
    for (int l = 0; l < levels; ++l) n += level_partials(planes, H, W, levels, l);
    return n;
}

extern "C" int ebfi_laploss_forward(const float *pred_a, const float *pred_b, const float *target, float coef_a, float coef_b,
                                    float *workspace, float *partial, int64_t planes_per_term, int H, int W, int levels,
                                    void *stream) {
    if (!pred_a || !target || !workspace || !partial) return fail(EBFI_ERR_ARG, "laploss_forward: null argument");
    if (!lap_dims_ok(planes_per_term, H, W, levels))
        return fail(EBFI_ERR_ARG, "laploss_forward: H, W must be multiples of 2^(levels-1) with >= 3 pixels on the coarsest blurred level");
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int64_t planes = planes_per_term * (pred_b ? 2 : 1);
    if (tiled_blocks(planes, H / 2, W / 2, RT) > 0x7fffffff) return fail(EBFI_ERR_ARG, "laploss_forward: too many planes");
    const int64_t n0 = planes_per_term * (int64_t)H * W;
    Coef cf{{coef_a, coef_b}, planes_per_term};
    float *cur = workspace;
    for (int l = 0; l + 1 < levels; ++l) {
        const int h = H >> l, w = W >> l;
        const int64_t n = planes * (int64_t)h * w;
        const int tyn = (int)tiles(h / 2, RT), txn = (int)tiles(w / 2, RT);
        const dim3 grid((unsigned)(planes * tyn * txn));
        // level 0 reads the images and writes the difference planes as well
        ProfScope ps("lap_reduce", st, 0.0, l == 0 ? 4.0 * n0 * (pred_b ? 3 : 2) + 5.0 * n : 5.0 * n);
        if (l == 0)
            hipLaunchKernelGGL(lap_reduce_kernel<true>, grid, dim3(LT), 0, st, nullptr, pred_a, pred_b, target, cur, cur + n,
                               planes_per_term, h, w, tyn, txn);
        else
            hipLaunchKernelGGL(lap_reduce_kernel<false>, grid, dim3(LT), 0, st, cur, nullptr, nullptr, nullptr, nullptr, cur + n,
                               planes_per_term, h, w, tyn, txn);
        cur += n;
    }
    cur = workspace;
    float *part = partial;
    for (int l = 0; l < levels; ++l) {
        const int h = H >> l, w = W >> l;
        const int64_t n = planes * (int64_t)h * w;
        const bool last = l + 1 == levels;
        const int64_t blocks = level_partials(planes, H, W, levels, l);
        ProfScope ps("lap_level", st, 0.0, (last ? 8.0 : 9.0) * n);
        if (last)
            hipLaunchKernelGGL(lap_last_kernel, dim3((unsigned)blocks), dim3(LT), 0, st, cur, part, n, (int64_t)h * w,
                               (float)(1 << l), cf);
        else
            hipLaunchKernelGGL(lap_level_kernel, dim3((unsigned)blocks), dim3(LT), 0, st, cur, cur + n, part, h, w,
                               (int)tiles(h, ET), (int)tiles(w, ET), (float)(1 << l), cf);
        part += blocks;
        cur += n;
    }
    return check_launch("laploss_forward");
}

extern "C" int ebfi_laploss_backward(const float *grad_loss, float *workspace, float *grad_pred, int64_t planes, int H, int W,
                                     int levels, void *stream) {
    if (!grad_loss || !workspace || !grad_pred) return fail(EBFI_ERR_ARG, "laploss_backward: null argument");
    if (!lap_dims_ok(planes, H, W, levels)) return fail(EBFI_ERR_ARG, "laploss_backward: bad dimensions");
    if (tiled_blocks(planes, H / 2, W / 2, RT) > 0x7fffffff) return fail(EBFI_ERR_ARG, "laploss_backward: too many planes");
    hipStream_t st = static_cast<hipStream_t>(stream);
    int64_t off[9];
    off[0] = 0;
    for (int l = 0; l < levels; ++l) off[l + 1] = off[l] + planes * (int64_t)(H >> l) * (W >> l);
    for (int l = levels - 2; l >= 0; --l) {
        const int h = H >> l, w = W >> l;
        const int64_t n = planes * (int64_t)h * w;
        float *s = workspace + off[l], *g = workspace + off[l + 1];
        {
            const int tyn = (int)tiles(h / 2, RT), txn = (int)tiles(w / 2, RT);
            ProfScope ps("lap_bwd_reduce", st, 0.0, 6.0 * n);
            hipLaunchKernelGGL(lap_bwd_reduce_kernel, dim3((unsigned)(planes * tyn * txn)), dim3(LT), 0, st, s, g, h, w, tyn, txn);
        }
        {
            const int tyn = (int)tiles(h, ET), txn = (int)tiles(w, ET);
            ProfScope ps("lap_bwd_expand", st, 0.0, 9.0 * n);
            hipLaunchKernelGGL(lap_bwd_expand_kernel, dim3((unsigned)(planes * tyn * txn)), dim3(LT), 0, st, s, g,
                               l == 0 ? grad_pred : s, l == 0 ? grad_loss : nullptr, h, w, tyn, txn);
        }
    }
    return check_launch("laploss_backward");
}
