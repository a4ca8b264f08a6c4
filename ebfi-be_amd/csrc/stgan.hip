// Everything between the convolutions of the STGAN adversarial loss (loss/adversarial.py, gan_type = 'STGAN', over
// loss/discriminator.py:208-263 of the reference): the sixteen 3x3 convolutions of the spatio-temporal patch discriminator are
// csrc/conv2d.hip's exact-fp32 kernels; what is here is the rest, as csrc/upsample.hip is for the Super-SloMo nets.  The law is
// written out in include/ebfi_hip.h (section "STGAN adversarial loss") and restated in float64 by tests/stgan_ref.py.
//
//   bn_lrelu forward / backward   training-mode BatchNorm2d + LeakyReLU on [B, C, H, W], running statistics in the same call
//   stgan_temporal forward / adj. [f1 - f0, f1 - f2] and its adjoint into f1, added to the spatial branch's gradient
//   linear forward / backward     the classifier's two skinny products, their data and weight gradients
//   bce_logits_pair               mean softplus(x_fake) + mean softplus(-x_real) and both gradients, device scalars
//   adamax_step                   torch.optim.Adamax over one flat buffer, the step count a device word
//
// Reductions.  A channel's B * H * W values are cut into chunks of kChunk; one workgroup folds one chunk -- every lane its quads
// in index order, then a fixed tree -- into ONE float64 pair in the workspace, and every workgroup of the pass that follows
// folds the channel's pairs again the same way (lane t takes pairs t, t + 256, ..., then the same tree).  The split depends on
// the shape only, nothing is accumulated atomically, and all sums are float64: two calls on the same data give the same bits,
// and a plane with mean 100 and spread 0.1 keeps its variance (x * x is exact in float64; the cancellation in E[x^2] - mean^2
// costs 1e-10 of it).  mean and rstd stay float64 (`stats`), so x - mean is taken before anything is rounded to float32.
//
// Streaming.  A lane owns quads of four adjacent elements: 16-byte loads and stores when H * W % 4 == 0 and the tensors are
// 16-byte aligned (a quad then never straddles two planes), scalar accesses otherwise; adamax and the temporal kernels take
// their n % 4 last elements by scalar accesses.
#include <cmath>

#include "common.hpp"

#pragma clang fp contract(off)

using namespace ebfi;

namespace {

constexpr int kThreads = 256;
constexpr int kChunk = EBFI_BN_CHUNK;                  // elements of one channel per workgroup: four quads per lane
constexpr int kQuadsPerLane = kChunk / (4 * kThreads);

struct f4 {
    float v[4];
};

__device__ inline f4 ld(const float *__restrict__ p, int64_t off, int lanes) {
    f4 r;
    if (lanes == 4) {
        const float4 q = *reinterpret_cast<const float4 *>(p + off);
        r.v[0] = q.x, r.v[1] = q.y, r.v[2] = q.z, r.v[3] = q.w;
    } else {
        r.v[0] = p[off];
        r.v[1] = r.v[2] = r.v[3] = 0.f;
    }
    return r;
}

__device__ inline void st(float *__restrict__ p, int64_t off, int lanes, const f4 &r) {
    if (lanes == 4)
        *reinterpret_cast<float4 *>(p + off) = make_float4(r.v[0], r.v[1], r.v[2], r.v[3]);
    else
        p[off] = r.v[0];
}

// Calls f(offset, lanes) for this lane's part of chunk s of channel c of a contiguous [B, C, HW] tensor, in index order:
// lanes == 4 (vec) one aligned quad, lanes == 1 one element.  n = B * HW.
template <class F>
__device__ inline void visit_chunk(int64_t n, int64_t HW, int C, int c, int64_t s, bool vec, F f) {
#pragma unroll
    for (int k = 0; k < kQuadsPerLane; ++k) {
        const int64_t j = s * kChunk + 4 * ((int64_t)threadIdx.x + (int64_t)kThreads * k);
        if (j >= n) break;
        if (vec) {
            const int64_t b = j / HW;
            f((b * C + c) * HW + (j - b * HW), 4);
        } else {
            for (int e = 0; e < 4 && j + e < n; ++e) {
                const int64_t b = (j + e) / HW;
                f((b * C + c) * HW + (j + e - b * HW), 1);
            }
        }
    }
}

// fixed tree over the workgroup; every lane leaves with both totals
__device__ inline void block_sum2(double &a, double &b, double *sh) {
    const int t = threadIdx.x;
    sh[t] = a;
    sh[kThreads + t] = b;
    __syncthreads();
    for (int o = kThreads / 2; o > 0; o >>= 1) {
        if (t < o) {
            sh[t] += sh[t + o];
            sh[kThreads + t] += sh[kThreads + t + o];
        }
        __syncthreads();
    }
    a = sh[0];
    b = sh[kThreads];
    __syncthreads();
}

// the channel's S pairs of the workspace, folded by the whole workgroup in a fixed order
__device__ inline void fold_pairs(const double *__restrict__ partial, int c, int64_t S, double &a, double &b, double *sh) {
    a = b = 0.0;
    for (int64_t i = threadIdx.x; i < S; i += kThreads) {
        a += partial[((int64_t)c * S + i) * 2];
        b += partial[((int64_t)c * S + i) * 2 + 1];
    }
    block_sum2(a, b, sh);
}

// ---------------------------------------------------------------------------------------------- BatchNorm + LeakyReLU
// grid (S, C): partial[(c * S + s) * 2 ..] = (sum x, sum x^2) of the chunk
__global__ __launch_bounds__(kThreads) void bn_stats_kernel(const float *__restrict__ x, double *__restrict__ partial, int64_t n,
                                                            int64_t HW, int C, int vec) {
    __shared__ double sh[2 * kThreads];
    const int c = blockIdx.y;
    const int64_t s = blockIdx.x, S = gridDim.x;
    double a = 0.0, q = 0.0;
    visit_chunk(n, HW, C, c, s, vec != 0, [&](int64_t off, int lanes) {
        const f4 v = ld(x, off, lanes);
        for (int e = 0; e < lanes; ++e) {
            const double d = (double)v.v[e];
            a += d;
            q += d * d;
        }
    });
    block_sum2(a, q, sh);
    if (threadIdx.x == 0) {
        partial[((int64_t)c * S + s) * 2] = a;
        partial[((int64_t)c * S + s) * 2 + 1] = q;
    }
}

__global__ __launch_bounds__(kThreads) void bn_apply_kernel(const float *__restrict__ x, const double *__restrict__ partial,
                                                            const float *__restrict__ gamma, const float *__restrict__ beta,
                                                            float *__restrict__ y, double *__restrict__ stats,
                                                            float *__restrict__ rmean, float *__restrict__ rvar,
                                                            int64_t *__restrict__ nbt, int64_t n, int64_t HW, int C, int vec,
                                                            double eps, double momentum, double slope) {
    __shared__ double sh[2 * kThreads];
    const int c = blockIdx.y;
    const int64_t s = blockIdx.x, S = gridDim.x;
    double a, q;
    fold_pairs(partial, c, S, a, q, sh);
    const double mean = a / (double)n;
    double var = q / (double)n - mean * mean;
    if (var < 0.0) var = 0.0;
    const double rstd = 1.0 / sqrt(var + eps);
    if (s == 0 && threadIdx.x == 0) {           // one writer per channel
        stats[2 * c] = mean;
        stats[2 * c + 1] = rstd;
        if (rmean != nullptr) {
            rmean[c] = (float)((1.0 - momentum) * (double)rmean[c] + momentum * mean);
            rvar[c] = (float)((1.0 - momentum) * (double)rvar[c] + momentum * (var * (double)n / (double)(n - 1)));
        }
        if (c == 0 && nbt != nullptr) nbt[0] += 1;
    }
    const double g = (double)gamma[c] * rstd, b = (double)beta[c];
    visit_chunk(n, HW, C, c, s, vec != 0, [&](int64_t off, int lanes) {
        f4 v = ld(x, off, lanes);
        for (int e = 0; e < lanes; ++e) {
            const double z = ((double)v.v[e] - mean) * g + b;
            v.v[e] = (float)(z > 0.0 ? z : z * slope);
        }
        st(y, off, lanes, v);
    });
}

// dy' = dy * LeakyReLU'(y) and xhat = (x - mean) * rstd of one element, float64
struct BwdElem {
    double g, xh;
};
__device__ inline BwdElem bwd_elem(float dy, float x, float y, double mean, double rstd, double slope) {
    return BwdElem{(double)dy * (y > 0.f ? 1.0 : slope), ((double)x - mean) * rstd};
}

__global__ __launch_bounds__(kThreads) void bn_bwd_sums_kernel(const float *__restrict__ dy, const float *__restrict__ x,
                                                               const float *__restrict__ y, const double *__restrict__ stats,
                                                               double *__restrict__ partial, int64_t n, int64_t HW, int C, int vec,
                                                               double slope) {
    __shared__ double sh[2 * kThreads];
    const int c = blockIdx.y;
    const int64_t s = blockIdx.x, S = gridDim.x;
    const double mean = stats[2 * c], rstd = stats[2 * c + 1];
    double a = 0.0, q = 0.0;
    visit_chunk(n, HW, C, c, s, vec != 0, [&](int64_t off, int lanes) {
        const f4 d = ld(dy, off, lanes), vx = ld(x, off, lanes), vy = ld(y, off, lanes);
        for (int e = 0; e < lanes; ++e) {
            const BwdElem r = bwd_elem(d.v[e], vx.v[e], vy.v[e], mean, rstd, slope);
            a += r.g;
            q += r.g * r.xh;
        }
    });
    block_sum2(a, q, sh);
    if (threadIdx.x == 0) {
        partial[((int64_t)c * S + s) * 2] = a;
        partial[((int64_t)c * S + s) * 2 + 1] = q;
    }
}

__global__ __launch_bounds__(kThreads) void bn_bwd_apply_kernel(const float *__restrict__ dy, const float *__restrict__ x,
                                                                const float *__restrict__ y, const float *__restrict__ gamma,
                                                                const double *__restrict__ stats, const double *__restrict__ partial,
                                                                float *__restrict__ dx, float *__restrict__ dgamma,
                                                                float *__restrict__ dbeta, int64_t n, int64_t HW, int C, int vec,
                                                                double slope) {
    __shared__ double sh[2 * kThreads];
    const int c = blockIdx.y;
    const int64_t s = blockIdx.x, S = gridDim.x;
    double s1, s2;
    fold_pairs(partial, c, S, s1, s2, sh);
    if (s == 0 && threadIdx.x == 0) {
        if (dgamma != nullptr) dgamma[c] = (float)s2;
        if (dbeta != nullptr) dbeta[c] = (float)s1;
    }
    const double mean = stats[2 * c], rstd = stats[2 * c + 1];
    const double k = (double)gamma[c] * rstd, m1 = s1 / (double)n, m2 = s2 / (double)n;
    visit_chunk(n, HW, C, c, s, vec != 0, [&](int64_t off, int lanes) {
        const f4 d = ld(dy, off, lanes), vx = ld(x, off, lanes), vy = ld(y, off, lanes);
        f4 o;
        for (int e = 0; e < lanes; ++e) {
            const BwdElem r = bwd_elem(d.v[e], vx.v[e], vy.v[e], mean, rstd, slope);
            o.v[e] = (float)(k * (r.g - m1 - r.xh * m2));
        }
        st(dx, off, lanes, o);
    });
}

// ---------------------------------------------------------------------------------------------- temporal input and its adjoint
// out [B, 2, CHW]: out[b, 0] = f1[b] - f0[b], out[b, 1] = f1[b] - f2[b]; per-sample strides in elements.  grid (quads, B)
__global__ __launch_bounds__(kThreads) void temporal_fwd_kernel(const float *__restrict__ f0, int64_t s0, const float *__restrict__ f1,
                                                                int64_t s1, const float *__restrict__ f2, int64_t s2,
                                                                float *__restrict__ out, int64_t CHW, int vec) {
    const int64_t b = blockIdx.y;
    const int64_t i = 4 * ((int64_t)blockIdx.x * kThreads + threadIdx.x);
    if (i >= CHW) return;
    const float *p0 = f0 + b * s0, *p1 = f1 + b * s1, *p2 = f2 + b * s2;
    float *oa = out + b * 2 * CHW, *ob = oa + CHW;
    if (vec && i + 4 <= CHW) {
        const f4 a = ld(p0, i, 4), m = ld(p1, i, 4), c = ld(p2, i, 4);
        f4 ra, rb;
        for (int e = 0; e < 4; ++e) ra.v[e] = m.v[e] - a.v[e], rb.v[e] = m.v[e] - c.v[e];
        st(oa, i, 4, ra);
        st(ob, i, 4, rb);
    } else {
        for (int64_t k = i; k < i + 4 && k < CHW; ++k) {
            oa[k] = p1[k] - p0[k];
            ob[k] = p1[k] - p2[k];
        }
    }
}

// grad_f1[b] = grad_t[b, 0] + grad_t[b, 1] (+ grad_s[b]), left to right
__global__ __launch_bounds__(kThreads) void temporal_bwd_kernel(const float *__restrict__ gt, const float *__restrict__ gs,
                                                                float *__restrict__ out, int64_t CHW, int vec) {
    const int64_t b = blockIdx.y;
    const int64_t i = 4 * ((int64_t)blockIdx.x * kThreads + threadIdx.x);
    if (i >= CHW) return;
    const float *ga = gt + b * 2 * CHW, *gb = ga + CHW, *s = gs ? gs + b * CHW : nullptr;
    float *o = out + b * CHW;
    if (vec && i + 4 <= CHW) {
        const f4 a = ld(ga, i, 4), c = ld(gb, i, 4);
        f4 r;
        for (int e = 0; e < 4; ++e) r.v[e] = a.v[e] + c.v[e];
        if (s) {
            const f4 d = ld(s, i, 4);
            for (int e = 0; e < 4; ++e) r.v[e] += d.v[e];
        }
        st(o, i, 4, r);
    } else {
        for (int64_t k = i; k < i + 4 && k < CHW; ++k) {
            float r = ga[k] + gb[k];
            if (s) r += s[k];
            o[k] = r;
        }
    }
}

// ---------------------------------------------------------------------------------------------- BCE with logits
// one workgroup: loss[0] = mean softplus(fake) + mean softplus(-real) (a NULL side contributes nothing), float64 sums in a fixed
// order; grad_fake = sigmoid(fake) / n, grad_real = (sigmoid(real) - 1) / n
__global__ __launch_bounds__(kThreads) void bce_pair_kernel(const float *__restrict__ fake, const float *__restrict__ real, int64_t n,
                                                            float *__restrict__ loss, float *__restrict__ gfake,
                                                            float *__restrict__ greal) {
    __shared__ double sh[2 * kThreads];
    double a = 0.0, b = 0.0;
    for (int64_t i = threadIdx.x; i < n; i += kThreads) {
        if (fake != nullptr) {
            const double x = (double)fake[i];
            a += fmax(x, 0.0) + log1p(exp(-fabs(x)));                      // target 0
            if (gfake != nullptr) gfake[i] = (float)((1.0 / (1.0 + exp(-x))) / (double)n);
        }
        if (real != nullptr) {
            const double x = (double)real[i];
            b += fmax(x, 0.0) - x + log1p(exp(-fabs(x)));                  // target 1
            if (greal != nullptr) greal[i] = (float)((1.0 / (1.0 + exp(-x)) - 1.0) / (double)n);
        }
    }
    block_sum2(a, b, sh);
    if (threadIdx.x == 0) loss[0] = (float)(a / (double)n + b / (double)n);
}

// ---------------------------------------------------------------------------------------------- Adamax
// torch.optim.Adamax, operation by operation in float32 (contraction off, an fma where add(alpha=) / lerp fuse):
//   g' = fma(p, wd, g);  m <- fma(1 - b1, g' - m, m);  u <- max(b2 u, |g'| + eps) (a NaN on either side stays);
//   p <- p - clr (m / u), clr = (float)(lr / (1 - b1^t)) with the bias correction in double, t = step[0]
struct AdamaxCoef {
    float w1, b2, eps, wd, clr;
};

template <bool WD>
__device__ inline void adamax_elem(float &p, float g, float &m, float &u, const AdamaxCoef &c) {
    if (WD) g = __builtin_fmaf(p, c.wd, g);
    m = __builtin_fmaf(c.w1, g - m, m);
    const float d = u * c.b2, r = fabsf(g) + c.eps;
    u = (d != d || d >= r) ? d : r;
    p = p - c.clr * (m / u);
}

template <bool WD>
__global__ __launch_bounds__(kThreads) void adamax_kernel(float *__restrict__ p, const float *__restrict__ g,
                                                          const float *__restrict__ g2, float *__restrict__ m, float *__restrict__ u,
                                                          const float *__restrict__ step, int64_t n4, int64_t n, double lr,
                                                          double beta1, double beta2, double eps, double wd) {
    const double t = (double)step[0];
    AdamaxCoef c;
    c.w1 = (float)(1.0 - beta1), c.b2 = (float)beta2, c.eps = (float)eps, c.wd = (float)wd;
    c.clr = (float)(lr / (1.0 - pow(beta1, t)));
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i < n4) {
        f4 P = ld(p, 4 * i, 4), M = ld(m, 4 * i, 4), U = ld(u, 4 * i, 4), G = ld(g, 4 * i, 4);
        if (g2 != nullptr) {
            const f4 H = ld(g2, 4 * i, 4);
            for (int e = 0; e < 4; ++e) G.v[e] += H.v[e];
        }
        for (int e = 0; e < 4; ++e) adamax_elem<WD>(P.v[e], G.v[e], M.v[e], U.v[e], c);
        st(p, 4 * i, 4, P);
        st(m, 4 * i, 4, M);
        st(u, 4 * i, 4, U);
    }
    if (i == 0)
        for (int64_t k = n4 * 4; k < n; ++k) adamax_elem<WD>(p[k], g2 != nullptr ? g[k] + g2[k] : g[k], m[k], u[k], c);
}

// ---------------------------------------------------------------------------------------------- the classifier's linear layers
// Skinny products (B rows against a [N, K] weight that is read once per kLinRows rows): every sum has ONE owner and a fixed
// order, so a captured step replays the bits of an eager one -- which a BLAS that picks its algorithm by the workspace it is
// given does not promise.
constexpr int kLinRows = 8;                     // batch rows per workgroup

// y[b, j] = act(sum_k x[b, k] w[j, k] + bias[j]); grid (N, ceil(B / kLinRows)); a lane takes quads k = 4 t, 4 (t + 256), ...
__global__ __launch_bounds__(kThreads) void linear_fwd_kernel(const float *__restrict__ x, const float *__restrict__ w,
                                                              const float *__restrict__ bias, float *__restrict__ y, int B, int64_t K,
                                                              int N, int vec, int act, float slope) {
    __shared__ float sh[kLinRows][kThreads];
    const int j = blockIdx.x, b0 = blockIdx.y * kLinRows, t = threadIdx.x;
    const int nb = B - b0 < kLinRows ? B - b0 : kLinRows;
    const float *wr = w + (int64_t)j * K;
    float acc[kLinRows];
#pragma unroll
    for (int r = 0; r < kLinRows; ++r) acc[r] = 0.f;
    if (vec) {
        for (int64_t k = 4 * (int64_t)t; k < K; k += 4 * kThreads) {
            const f4 W = ld(wr, k, 4);
#pragma unroll
            for (int r = 0; r < kLinRows; ++r)
                if (r < nb) {
                    const f4 X = ld(x, (int64_t)(b0 + r) * K + k, 4);
                    for (int e = 0; e < 4; ++e) acc[r] = __builtin_fmaf(W.v[e], X.v[e], acc[r]);
                }
        }
    } else {
        for (int64_t k = t; k < K; k += kThreads) {
            const float wv = wr[k];
#pragma unroll
            for (int r = 0; r < kLinRows; ++r)
                if (r < nb) acc[r] = __builtin_fmaf(wv, x[(int64_t)(b0 + r) * K + k], acc[r]);
        }
    }
#pragma unroll
    for (int r = 0; r < kLinRows; ++r) sh[r][t] = acc[r];
    __syncthreads();
    for (int o = kThreads / 2; o > 0; o >>= 1) {
        if (t < o)
            for (int r = 0; r < nb; ++r) sh[r][t] += sh[r][t + o];
        __syncthreads();
    }
    if (t < nb) {
        float v = sh[t][0] + (bias != nullptr ? bias[j] : 0.f);
        if (act && !(v > 0.f)) v = v * slope;
        y[(int64_t)(b0 + t) * N + j] = v;
    }
}

// gx[b, k] = (sum_j gy[b, j] w[j, k]) * (mask == NULL ? 1 : mask[b, k] > 0 ? 1 : slope); a workgroup owns 64 columns k and
// splits the rows j over four lane groups, folded 0 + 1 + 2 + 3; grid (ceil(K / 64), ceil(B / kLinRows))
__global__ __launch_bounds__(kThreads) void linear_bwd_data_kernel(const float *__restrict__ gy, const float *__restrict__ w,
                                                                   const float *__restrict__ mask, float *__restrict__ gx, int B,
                                                                   int64_t K, int N, float slope) {
    __shared__ float sh[4][kLinRows][64];
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6, b0 = blockIdx.y * kLinRows;
    const int nb = B - b0 < kLinRows ? B - b0 : kLinRows;
    const int64_t k = (int64_t)blockIdx.x * 64 + tx;
    const int per = (N + 3) / 4, j0 = ty * per, j1 = j0 + per < N ? j0 + per : N;
    float acc[kLinRows];
#pragma unroll
    for (int r = 0; r < kLinRows; ++r) acc[r] = 0.f;
    if (k < K)
        for (int j = j0; j < j1; ++j) {
            const float wv = w[(int64_t)j * K + k];
#pragma unroll
            for (int r = 0; r < kLinRows; ++r)
                if (r < nb) acc[r] = __builtin_fmaf(gy[(int64_t)(b0 + r) * N + j], wv, acc[r]);
        }
#pragma unroll
    for (int r = 0; r < kLinRows; ++r) sh[ty][r][tx] = acc[r];
    __syncthreads();
    if (ty == 0 && k < K)
        for (int r = 0; r < nb; ++r) {
            float v = ((sh[0][r][tx] + sh[1][r][tx]) + sh[2][r][tx]) + sh[3][r][tx];
            const int64_t o = (int64_t)(b0 + r) * K + k;
            if (mask != nullptr && !(mask[o] > 0.f)) v = v * slope;
            gx[o] = v;
        }
}

// The same for K % 4 == 0 and 16-byte aligned tensors: a lane owns FOUR columns (one 16-byte load per weight row), sixteen lanes
// 64 columns, and the rows j are split over sixteen lane groups, folded 0 + 1 + ... + 15; grid as above
constexpr int kDGroups = 16;
__global__ __launch_bounds__(kThreads) void linear_bwd_data_vec_kernel(const float *__restrict__ gy, const float *__restrict__ w,
                                                                       const float *__restrict__ mask, float *__restrict__ gx, int B,
                                                                       int64_t K, int N, float slope) {
    __shared__ float sh[kDGroups][kLinRows][64];
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4, b0 = blockIdx.y * kLinRows;
    const int nb = B - b0 < kLinRows ? B - b0 : kLinRows;
    const int64_t k = (int64_t)blockIdx.x * 64 + 4 * tx;
    const int per = (N + kDGroups - 1) / kDGroups, j0 = ty * per, j1 = j0 + per < N ? j0 + per : N;
    f4 acc[kLinRows];
#pragma unroll
    for (int r = 0; r < kLinRows; ++r) acc[r].v[0] = acc[r].v[1] = acc[r].v[2] = acc[r].v[3] = 0.f;
    if (k < K)
        for (int j = j0; j < j1; ++j) {
            const f4 W = ld(w, (int64_t)j * K + k, 4);
#pragma unroll
            for (int r = 0; r < kLinRows; ++r)
                if (r < nb) {
                    const float g = gy[(int64_t)(b0 + r) * N + j];
                    for (int e = 0; e < 4; ++e) acc[r].v[e] = __builtin_fmaf(g, W.v[e], acc[r].v[e]);
                }
        }
#pragma unroll
    for (int r = 0; r < kLinRows; ++r)
        for (int e = 0; e < 4; ++e) sh[ty][r][4 * tx + e] = acc[r].v[e];
    __syncthreads();
    for (int o = threadIdx.x; o < kLinRows * 64; o += kThreads) {
        const int r = o >> 6, c = o & 63;
        const int64_t kk = (int64_t)blockIdx.x * 64 + c;
        if (r < nb && kk < K) {
            float v = sh[0][r][c];
            for (int g = 1; g < kDGroups; ++g) v += sh[g][r][c];
            const int64_t at = (int64_t)(b0 + r) * K + kk;
            if (mask != nullptr && !(mask[at] > 0.f)) v = v * slope;
            gx[at] = v;
        }
    }
}

// gw[j, k] = sum_b gy[b, j] x[b, k] (b in order), gb[j] = sum_b gy[b, j]; a lane owns one quad of k for kWRows rows j, so a
// row of x is read once per kWRows rows of the gradient; grid (ceil(ceil(K / 4) / 256), ceil(N / kWRows))
constexpr int kWRows = 16;
__global__ __launch_bounds__(kThreads) void linear_bwd_weight_kernel(const float *__restrict__ gy, const float *__restrict__ x,
                                                                     float *__restrict__ gw, float *__restrict__ gb, int B, int64_t K,
                                                                     int N, int vec) {
    const int j0 = blockIdx.y * kWRows;
    const int nj = N - j0 < kWRows ? N - j0 : kWRows;
    if (gb != nullptr && blockIdx.x == 0 && (int)threadIdx.x < nj) {
        float s = 0.f;
        for (int b = 0; b < B; ++b) s += gy[(int64_t)b * N + j0 + threadIdx.x];
        gb[j0 + threadIdx.x] = s;
    }
    const int64_t k = 4 * ((int64_t)blockIdx.x * kThreads + threadIdx.x);
    if (k >= K) return;
    if (vec) {
        f4 acc[kWRows];
#pragma unroll
        for (int jj = 0; jj < kWRows; ++jj) acc[jj].v[0] = acc[jj].v[1] = acc[jj].v[2] = acc[jj].v[3] = 0.f;
        for (int b = 0; b < B; ++b) {
            const f4 X = ld(x, (int64_t)b * K + k, 4);
#pragma unroll
            for (int jj = 0; jj < kWRows; ++jj)
                if (jj < nj) {
                    const float g = gy[(int64_t)b * N + j0 + jj];
                    for (int e = 0; e < 4; ++e) acc[jj].v[e] = __builtin_fmaf(g, X.v[e], acc[jj].v[e]);
                }
        }
#pragma unroll
        for (int jj = 0; jj < kWRows; ++jj)
            if (jj < nj) st(gw, (int64_t)(j0 + jj) * K + k, 4, acc[jj]);
    } else {
        for (int64_t kk = k; kk < k + 4 && kk < K; ++kk)
            for (int jj = 0; jj < nj; ++jj) {
                float a = 0.f;
                for (int b = 0; b < B; ++b) a = __builtin_fmaf(gy[(int64_t)b * N + j0 + jj], x[(int64_t)b * K + kk], a);
                gw[(int64_t)(j0 + jj) * K + kk] = a;
            }
    }
}

int check_linear(const char *what, int64_t B, int64_t K, int64_t N) {
    if (B < 1 || K < 1 || N < 1) return fail(EBFI_ERR_ARG, "%s: B = %lld, K = %lld, N = %lld must be positive", what, (long long)B, (long long)K, (long long)N);
    if (B > 8 * 65535 || N > 65535 || K > ((int64_t)1 << 31) - 1)
        return fail(EBFI_ERR_UNSUPPORTED, "%s: B = %lld, K = %lld, N = %lld beyond the grid (B <= 524280, N <= 65535, K < 2^31)", what, (long long)B,
                    (long long)K, (long long)N);
    return EBFI_OK;
}

int check_bn(const char *what, int64_t B, int C, int64_t HW, int64_t *S) {
    if (B < 1 || C < 1 || HW < 1) return fail(EBFI_ERR_ARG, "%s: B = %lld, C = %d, H*W = %lld must be positive", what, (long long)B, C, (long long)HW);
    if (B > ((int64_t)1 << 40) / HW) return fail(EBFI_ERR_UNSUPPORTED, "%s: B * H*W too large", what);
    if (B * HW < 2)
        return fail(EBFI_ERR_ARG, "%s: batch statistics need more than 1 value per channel (B * H*W = 1), as torch refuses it", what);
    if (C > 65535) return fail(EBFI_ERR_UNSUPPORTED, "%s: C = %d beyond 65535", what, C);
    *S = ceil_div(B * HW, kChunk);
    if (*S > 0x7fffffff) return fail(EBFI_ERR_UNSUPPORTED, "%s: a grid beyond 2^31 - 1", what);
    return EBFI_OK;
}

}  // namespace

extern "C" int64_t ebfi_bn_lrelu_workspace(int64_t B, int C, int64_t HW) {
    if (B < 1 || C < 1 || HW < 1) return 0;
    return ceil_div(B * HW, kChunk) * C * 2 * (int64_t)sizeof(double);
}

extern "C" int ebfi_bn_lrelu_forward(const float *x, const float *gamma, const float *beta, float *y, double *stats,
                                     float *running_mean, float *running_var, int64_t *num_batches_tracked, int64_t B, int C,
                                     int64_t HW, double eps, double momentum, double slope, void *workspace, int64_t workspace_bytes,
                                     void *stream) {
    if (!x || !gamma || !beta || !y || !stats) return fail(EBFI_ERR_ARG, "bn_lrelu_forward: null pointer");
    if ((running_mean == nullptr) != (running_var == nullptr))
        return fail(EBFI_ERR_ARG, "bn_lrelu_forward: running_mean and running_var come together");
    int64_t S = 0;
    if (int rc = check_bn("bn_lrelu_forward", B, C, HW, &S)) return rc;
    if (!(eps >= 0.0) || !(momentum >= 0.0 && momentum <= 1.0)) return fail(EBFI_ERR_ARG, "bn_lrelu_forward: eps = %g, momentum = %g", eps, momentum);
    if (!workspace || workspace_bytes < ebfi_bn_lrelu_workspace(B, C, HW) || (reinterpret_cast<uintptr_t>(workspace) & 7u))
        return fail(EBFI_ERR_WORKSPACE, "bn_lrelu_forward: workspace missing, misaligned or below %lld bytes", (long long)ebfi_bn_lrelu_workspace(B, C, HW));
    const int vec = HW % 4 == 0 && aligned16(x) && aligned16(y);
    const int64_t n = B * HW;
    double *partial = static_cast<double *>(workspace);
    hipStream_t stq = static_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)S, (unsigned)C);
    {
        ProfScope ps_("bn_stats", stq, 0.0, 4.0 * (double)n * C);
        hipLaunchKernelGGL(bn_stats_kernel, grid, dim3(kThreads), 0, stq, x, partial, n, HW, C, vec);
    }
    if (int rc = check_launch("bn_lrelu_forward (statistics)")) return rc;
    {
        ProfScope ps_("bn_lrelu_apply", stq, 0.0, 8.0 * (double)n * C);
        hipLaunchKernelGGL(bn_apply_kernel, grid, dim3(kThreads), 0, stq, x, partial, gamma, beta, y, stats, running_mean, running_var,
                           num_batches_tracked, n, HW, C, vec, eps, momentum, slope);
    }
    return check_launch("bn_lrelu_forward");
}

extern "C" int ebfi_bn_lrelu_backward(const float *grad_y, const float *x, const float *y, const float *gamma, const double *stats,
                                      float *grad_x, float *grad_gamma, float *grad_beta, int64_t B, int C, int64_t HW, double slope,
                                      void *workspace, int64_t workspace_bytes, void *stream) {
    if (!grad_y || !x || !y || !gamma || !stats || !grad_x) return fail(EBFI_ERR_ARG, "bn_lrelu_backward: null pointer");
    int64_t S = 0;
    if (int rc = check_bn("bn_lrelu_backward", B, C, HW, &S)) return rc;
    if (!workspace || workspace_bytes < ebfi_bn_lrelu_workspace(B, C, HW) || (reinterpret_cast<uintptr_t>(workspace) & 7u))
        return fail(EBFI_ERR_WORKSPACE, "bn_lrelu_backward: workspace missing, misaligned or below %lld bytes", (long long)ebfi_bn_lrelu_workspace(B, C, HW));
    const int vec = HW % 4 == 0 && aligned16(grad_y) && aligned16(x) && aligned16(y) && aligned16(grad_x);
    const int64_t n = B * HW;
    double *partial = static_cast<double *>(workspace);
    hipStream_t stq = static_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)S, (unsigned)C);
    {
        ProfScope ps_("bn_lrelu_bwd_sums", stq, 0.0, 12.0 * (double)n * C);
        hipLaunchKernelGGL(bn_bwd_sums_kernel, grid, dim3(kThreads), 0, stq, grad_y, x, y, stats, partial, n, HW, C, vec, slope);
    }
    if (int rc = check_launch("bn_lrelu_backward (sums)")) return rc;
    {
        ProfScope ps_("bn_lrelu_bwd_apply", stq, 0.0, 16.0 * (double)n * C);
        hipLaunchKernelGGL(bn_bwd_apply_kernel, grid, dim3(kThreads), 0, stq, grad_y, x, y, gamma, stats, partial, grad_x, grad_gamma,
                           grad_beta, n, HW, C, vec, slope);
    }
    return check_launch("bn_lrelu_backward");
}

extern "C" int ebfi_stgan_temporal_forward(const float *f0, int64_t f0_stride, const float *f1, int64_t f1_stride, const float *f2,
                                           int64_t f2_stride, float *out, int64_t B, int64_t CHW, void *stream) {
    if (!f0 || !f1 || !f2 || !out) return fail(EBFI_ERR_ARG, "stgan_temporal_forward: null pointer");
    if (B < 1 || CHW < 1 || B > 65535) return fail(EBFI_ERR_ARG, "stgan_temporal_forward: B = %lld (1 .. 65535), C*H*W = %lld", (long long)B, (long long)CHW);
    if (f0_stride < CHW || f1_stride < CHW || f2_stride < CHW) return fail(EBFI_ERR_ARG, "stgan_temporal_forward: a sample stride below C*H*W");
    const int64_t blocks = ceil_div(ceil_div(CHW, 4), kThreads);
    if (blocks > 0x7fffffff) return fail(EBFI_ERR_UNSUPPORTED, "stgan_temporal_forward: a grid beyond 2^31 - 1");
    const int vec = CHW % 4 == 0 && f0_stride % 4 == 0 && f1_stride % 4 == 0 && f2_stride % 4 == 0 && aligned16(f0) && aligned16(f1) &&
                    aligned16(f2) && aligned16(out);
    hipStream_t stq = static_cast<hipStream_t>(stream);
    {
        ProfScope ps_("stgan_temporal_fwd", stq, 0.0, 20.0 * (double)B * CHW);
        hipLaunchKernelGGL(temporal_fwd_kernel, dim3((unsigned)blocks, (unsigned)B), dim3(kThreads), 0, stq, f0, f0_stride, f1, f1_stride,
                           f2, f2_stride, out, CHW, vec);
    }
    return check_launch("stgan_temporal_forward");
}

extern "C" int ebfi_stgan_temporal_backward(const float *grad_t, const float *grad_s, float *grad_f1, int64_t B, int64_t CHW,
                                            void *stream) {
    if (!grad_t || !grad_f1) return fail(EBFI_ERR_ARG, "stgan_temporal_backward: null pointer");
    if (B < 1 || CHW < 1 || B > 65535) return fail(EBFI_ERR_ARG, "stgan_temporal_backward: B = %lld (1 .. 65535), C*H*W = %lld", (long long)B, (long long)CHW);
    const int64_t blocks = ceil_div(ceil_div(CHW, 4), kThreads);
    if (blocks > 0x7fffffff) return fail(EBFI_ERR_UNSUPPORTED, "stgan_temporal_backward: a grid beyond 2^31 - 1");
    const int vec = CHW % 4 == 0 && aligned16(grad_t) && aligned16(grad_f1) && (!grad_s || aligned16(grad_s));
    hipStream_t stq = static_cast<hipStream_t>(stream);
    {
        ProfScope ps_("stgan_temporal_bwd", stq, 0.0, (grad_s ? 16.0 : 12.0) * (double)B * CHW);
        hipLaunchKernelGGL(temporal_bwd_kernel, dim3((unsigned)blocks, (unsigned)B), dim3(kThreads), 0, stq, grad_t, grad_s, grad_f1, CHW, vec);
    }
    return check_launch("stgan_temporal_backward");
}

extern "C" int ebfi_bce_logits_pair(const float *fake, const float *real, int64_t n, float *loss, float *grad_fake, float *grad_real,
                                    void *stream) {
    if (!loss || (!fake && !real)) return fail(EBFI_ERR_ARG, "bce_logits_pair: null pointer");
    if ((grad_fake && !fake) || (grad_real && !real)) return fail(EBFI_ERR_ARG, "bce_logits_pair: a gradient without its logits");
    if (n < 1) return fail(EBFI_ERR_ARG, "bce_logits_pair: n = %lld", (long long)n);
    hipStream_t stq = static_cast<hipStream_t>(stream);
    {
        ProfScope ps_("bce_logits_pair", stq, 0.0, 16.0 * (double)n);
        hipLaunchKernelGGL(bce_pair_kernel, dim3(1), dim3(kThreads), 0, stq, fake, real, n, loss, grad_fake, grad_real);
    }
    return check_launch("bce_logits_pair");
}

extern "C" int ebfi_linear_forward(const float *x, const float *weight, const float *bias, float *y, int64_t B, int64_t K, int64_t N,
                                   int act, double slope, void *stream) {
    if (!x || !weight || !y) return fail(EBFI_ERR_ARG, "linear_forward: null pointer");
    if (int rc = check_linear("linear_forward", B, K, N)) return rc;
    if (act != 0 && act != 1) return fail(EBFI_ERR_ARG, "linear_forward: act = %d (0 none, 1 LeakyReLU)", act);
    const int vec = K % 4 == 0 && aligned16(x) && aligned16(weight);
    hipStream_t stq = static_cast<hipStream_t>(stream);
    {
        ProfScope ps_("linear_fwd", stq, 2.0 * B * (double)K * N, 4.0 * ((double)N * K + (double)B * (K + N)));
        hipLaunchKernelGGL(linear_fwd_kernel, dim3((unsigned)N, (unsigned)ceil_div(B, kLinRows)), dim3(kThreads), 0, stq, x, weight, bias, y,
                           (int)B, K, (int)N, vec, act, (float)slope);
    }
    return check_launch("linear_forward");
}

extern "C" int ebfi_linear_backward_data(const float *grad_y, const float *weight, const float *mask_y, double slope, float *grad_x,
                                         int64_t B, int64_t K, int64_t N, void *stream) {
    if (!grad_y || !weight || !grad_x) return fail(EBFI_ERR_ARG, "linear_backward_data: null pointer");
    if (int rc = check_linear("linear_backward_data", B, K, N)) return rc;
    hipStream_t stq = static_cast<hipStream_t>(stream);
    {
        ProfScope ps_("linear_bwd_data", stq, 2.0 * B * (double)K * N, 4.0 * ((double)N * K + (double)B * (K + N)));
        const dim3 grid((unsigned)ceil_div(K, 64), (unsigned)ceil_div(B, kLinRows));
        if (K % 4 == 0 && aligned16(weight))
            hipLaunchKernelGGL(linear_bwd_data_vec_kernel, grid, dim3(kThreads), 0, stq, grad_y, weight, mask_y, grad_x, (int)B, K, (int)N,
                               (float)slope);
        else
            hipLaunchKernelGGL(linear_bwd_data_kernel, grid, dim3(kThreads), 0, stq, grad_y, weight, mask_y, grad_x, (int)B, K, (int)N,
                               (float)slope);
    }
    return check_launch("linear_backward_data");
}

extern "C" int ebfi_linear_backward_weight(const float *grad_y, const float *x, float *grad_weight, float *grad_bias, int64_t B,
                                           int64_t K, int64_t N, void *stream) {
    if (!grad_y || !x || !grad_weight) return fail(EBFI_ERR_ARG, "linear_backward_weight: null pointer");
    if (int rc = check_linear("linear_backward_weight", B, K, N)) return rc;
    const int vec = K % 4 == 0 && aligned16(x) && aligned16(grad_weight);
    hipStream_t stq = static_cast<hipStream_t>(stream);
    {
        ProfScope ps_("linear_bwd_weight", stq, 2.0 * B * (double)K * N, 4.0 * ((double)N * K + (double)B * (K + N)));
        hipLaunchKernelGGL(linear_bwd_weight_kernel, dim3((unsigned)ceil_div(ceil_div(K, 4), kThreads), (unsigned)ceil_div(N, kWRows)),
                           dim3(kThreads), 0, stq, grad_y, x, grad_weight, grad_bias, (int)B, K, (int)N, vec);
    }
    return check_launch("linear_backward_weight");
}

extern "C" int ebfi_adamax_step(float *param, const float *grad, const float *grad2, float *exp_avg, float *exp_inf, const float *step,
                                int64_t n, double lr, double beta1, double beta2, double eps, double weight_decay, void *stream) {
    if (!param || !grad || !exp_avg || !exp_inf || !step) return fail(EBFI_ERR_ARG, "adamax_step: null pointer");
    if (n < 1) return fail(EBFI_ERR_ARG, "adamax_step: n = %lld", (long long)n);
    if (!(lr >= 0.0) || !(beta1 >= 0.0 && beta1 < 1.0) || !(beta2 >= 0.0 && beta2 < 1.0) || !(eps >= 0.0) || !(weight_decay >= 0.0))
        return fail(EBFI_ERR_ARG, "adamax_step: lr = %g, betas = (%g, %g), eps = %g, weight_decay = %g", lr, beta1, beta2, eps, weight_decay);
    if (!aligned16(param) || !aligned16(grad) || !aligned16(exp_avg) || !aligned16(exp_inf) || (grad2 && !aligned16(grad2)))
        return fail(EBFI_ERR_ARG, "adamax_step: buffers must be 16-byte aligned");
    const int64_t n4 = n / 4;
    const int64_t blocks = ceil_div(n4 > 0 ? n4 : 1, kThreads);
    if (blocks > 0x7fffffff) return fail(EBFI_ERR_UNSUPPORTED, "adamax_step: a grid beyond 2^31 - 1");
    hipStream_t stq = static_cast<hipStream_t>(stream);
    {
        ProfScope ps_("adamax_step", stq, 0.0, 4.0 * (double)n * (grad2 ? 8.0 : 7.0));
        if (weight_decay != 0.0)
            hipLaunchKernelGGL(adamax_kernel<true>, dim3((unsigned)blocks), dim3(kThreads), 0, stq, param, grad, grad2, exp_avg, exp_inf, step,
                               n4, n, lr, beta1, beta2, eps, weight_decay);
        else
            hipLaunchKernelGGL(adamax_kernel<false>, dim3((unsigned)blocks), dim3(kThreads), 0, stq, param, grad, grad2, exp_avg, exp_inf, step,
                               n4, n, lr, beta1, beta2, eps, weight_decay);
    }
    return check_launch("adamax_step");
}
