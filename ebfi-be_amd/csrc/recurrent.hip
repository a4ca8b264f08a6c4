// The parts between the convolutions of models/model_misc/unet.py's recurrent U-Nets (UNetFlow, UNetRecurrent, SRUNetRecurrent):
// the ConvLSTM and ConvGRU cell tails of models/model_misc/submodules.py and the bilinear x2 / x4 up-sampling of
// UpsampleConvLayer, each with its gradient.  The convolutions are csrc/conv2d.hip's.  The law is written out in
// include/ebfi_hip.h (ebfi_lstm_cell_*, ebfi_gru_*, ebfi_bilinear_up_*) and restated in float64 by tests/unet_ref.py.
//
//   lstm_cell_forward    gates [B, 4C, HW] (in, remember, out, cell), prev_cell -> hidden, cell: one pass, 7 C floats per pixel
//   lstm_cell_backward   recomputes the three sigmoids and both tanh from the saved pre-activations: nothing but `cell` is kept
//   gru_reset_forward    cat(x, h * sigmoid(reset)) written straight into the [B, Cx + C, HW] input of the out-gate convolution
//   gru_update_forward   h * (1 - sigmoid(update)) + tanh(out) * sigmoid(update)
//   gru_*_backward       the gradients of the three pre-activations, of h (both halves) and of x through the written cat
//   bilinear_up_forward  F.interpolate(scale_factor = 2 | 4, mode = 'bilinear', align_corners = False)
//   bilinear_up_backward its adjoint as a GATHER: an input pixel adds its (at most 2 scale)^2 contributors row by row, left to
//                        right, in float32 -- a fixed order, so the result is bit-reproducible.  No atomics in this file.
//
// Streaming kernels: a lane owns FOUR adjacent pixels of one plane, so every access is a 16-byte load or store when HW % 4 == 0
// and the tensors are 16-byte aligned; otherwise (an odd plane offset breaks the alignment of every plane) the same lane makes
// scalar accesses below HW.  The grid is capped at kMaxBlocks workgroups and strides over the rest.  expf, tanhf and the
// division are hipcc's accurate defaults; contraction is off so that the float32 order is the one written here.  The
// derivatives s (1 - s) and 1 - tanh^2 are formed without the subtraction (sig2, sech2 below): a saturated gate keeps its
// relative accuracy, which the expression 1 - s in float32 does not.
#include <cmath>
#include <initializer_list>

#include "common.hpp"

#pragma clang fp contract(off)

using namespace ebfi;

namespace {

constexpr int kThreads = 256;
constexpr int kMaxBlocks = 2048;      // 256 CUs x 8 workgroups: larger maps stride

struct f4 {
    float v[4];
};

// four consecutive floats at p[i .. i + 3]; `vec`: one 16-byte access (i % 4 == 0, p + i aligned); else scalar accesses below `n`
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

__device__ inline f4 zero4() {
    f4 r;
#pragma unroll
    for (int k = 0; k < 4; ++k) r.v[k] = 0.f;
    return r;
}

// p == nullptr reads zeros
__device__ inline f4 load4_opt(const float *__restrict__ p, int64_t i, int64_t n, bool vec) { return p ? load4(p, i, n, vec) : zero4(); }

__device__ inline void store4(float *__restrict__ p, int64_t i, int64_t n, bool vec, const f4 &r) {
    if (vec) {
        *reinterpret_cast<float4 *>(p + i) = make_float4(r.v[0], r.v[1], r.v[2], r.v[3]);
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (i + k < n) p[i + k] = r.v[k];
    }
}

// sigmoid(x) and 1 - sigmoid(x) = sigmoid(-x), both from e = exp(-|x|) <= 1: no overflow, and the complement is not formed by a
// subtraction from 1, which would lose it (and with it the derivative s * c) once the gate saturates
struct Sig {
    float s, c;
};

__device__ inline Sig sig2(float x) {
    const float e = expf(-fabsf(x));
    const float p = 1.f / (1.f + e), q = e / (1.f + e);
    return x >= 0.f ? Sig{p, q} : Sig{q, p};
}

// 1 - tanh(x)^2 with t = tanh(x): past |x| = 0.625 (t^2 > 0.3) as 4 e / (1 + e)^2, e = exp(-2 |x|), for the same reason
__device__ inline float sech2(float x, float t) {
    const float ax = fabsf(x);
    if (!(ax >= 0.625f)) return 1.f - t * t;
    const float e = expf(-2.f * ax), d = 1.f + e;
    return 4.f * e / (d * d);
}

// ---------------------------------------------------------------------------------------------- ConvLSTM
// items: B * C planes x ceil(HW / 4) quads
__global__ __launch_bounds__(kThreads) void lstm_cell_fwd_kernel(const float *__restrict__ gates, const float *__restrict__ prev_cell,
                                                                 float *__restrict__ hidden, float *__restrict__ cell, int64_t planes,
                                                                 int C, int64_t HW, int vec) {
    const int64_t nq = (HW + 3) / 4, total = planes * nq, gs = (int64_t)C * HW;
    for (int64_t id = (int64_t)blockIdx.x * kThreads + threadIdx.x; id < total; id += (int64_t)gridDim.x * kThreads) {
        const int64_t plane = id / nq, i = 4 * (id - plane * nq);
        const int64_t b = plane / C, c = plane - b * C;
        const float *g = gates + (b * 4 * C + c) * HW;
        const f4 gi = load4(g, i, HW, vec), gf = load4(g + gs, i, HW, vec), go = load4(g + 2 * gs, i, HW, vec),
                 gc = load4(g + 3 * gs, i, HW, vec);
        const f4 cp = load4_opt(prev_cell ? prev_cell + plane * HW : nullptr, i, HW, vec);
        f4 h, cl;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float in = sig2(gi.v[k]).s, rem = sig2(gf.v[k]).s, out = sig2(go.v[k]).s, cg = tanhf(gc.v[k]);
            cl.v[k] = rem * cp.v[k] + in * cg;
            h.v[k] = out * tanhf(cl.v[k]);
        }
        store4(hidden + plane * HW, i, HW, vec, h);
        store4(cell + plane * HW, i, HW, vec, cl);
    }
}

__global__ __launch_bounds__(kThreads) void lstm_cell_bwd_kernel(const float *__restrict__ gates, const float *__restrict__ prev_cell,
                                                                 const float *__restrict__ cell, const float *__restrict__ grad_hidden,
                                                                 const float *__restrict__ grad_cell, float *__restrict__ grad_gates,
                                                                 float *__restrict__ grad_prev_cell, int64_t planes, int C, int64_t HW,
                                                                 int vec) {
    const int64_t nq = (HW + 3) / 4, total = planes * nq, gs = (int64_t)C * HW;
    for (int64_t id = (int64_t)blockIdx.x * kThreads + threadIdx.x; id < total; id += (int64_t)gridDim.x * kThreads) {
        const int64_t plane = id / nq, i = 4 * (id - plane * nq);
        const int64_t b = plane / C, c = plane - b * C;
        const int64_t goff = (b * 4 * C + c) * HW;
        const float *g = gates + goff;
        const f4 gi = load4(g, i, HW, vec), gf = load4(g + gs, i, HW, vec), go = load4(g + 2 * gs, i, HW, vec),
                 gc = load4(g + 3 * gs, i, HW, vec);
        const f4 cp = load4_opt(prev_cell ? prev_cell + plane * HW : nullptr, i, HW, vec);
        const f4 cl = load4(cell + plane * HW, i, HW, vec);
        const f4 gh = load4_opt(grad_hidden ? grad_hidden + plane * HW : nullptr, i, HW, vec);
        const f4 gcl = load4_opt(grad_cell ? grad_cell + plane * HW : nullptr, i, HW, vec);
        f4 di, df, dout, dg, dcp;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const Sig in = sig2(gi.v[k]), rem = sig2(gf.v[k]), out = sig2(go.v[k]);
            const float cg = tanhf(gc.v[k]), tc = tanhf(cl.v[k]);
            const float dcell = gcl.v[k] + gh.v[k] * out.s * sech2(cl.v[k], tc);
            dout.v[k] = gh.v[k] * tc * (out.s * out.c);
            di.v[k] = dcell * cg * (in.s * in.c);
            df.v[k] = dcell * cp.v[k] * (rem.s * rem.c);
            dg.v[k] = dcell * in.s * sech2(gc.v[k], cg);
            dcp.v[k] = dcell * rem.s;
        }
        float *d = grad_gates + goff;
        store4(d, i, HW, vec, di);
        store4(d + gs, i, HW, vec, df);
        store4(d + 2 * gs, i, HW, vec, dout);
        store4(d + 3 * gs, i, HW, vec, dg);
        if (grad_prev_cell) store4(grad_prev_cell + plane * HW, i, HW, vec, dcp);
    }
}

// ---------------------------------------------------------------------------------------------- ConvGRU
// items: B * (Cx + C) planes of `out` x quads; a plane below Cx copies x, the others write h * sigmoid(reset)
__global__ __launch_bounds__(kThreads) void gru_reset_fwd_kernel(const float *__restrict__ reset_pre, const float *__restrict__ x,
                                                                 const float *__restrict__ h, float *__restrict__ out, int64_t B, int Cx,
                                                                 int C, int64_t HW, int vec) {
    const int Ct = Cx + C;
    const int64_t nq = (HW + 3) / 4, total = B * Ct * nq;
    for (int64_t id = (int64_t)blockIdx.x * kThreads + threadIdx.x; id < total; id += (int64_t)gridDim.x * kThreads) {
        const int64_t plane = id / nq, i = 4 * (id - plane * nq);
        const int64_t b = plane / Ct, c = plane - b * Ct;
        f4 o;
        if (c < Cx) {
            o = load4(x + (b * Cx + c) * HW, i, HW, vec);
        } else if (h) {
            const int64_t hp = (b * C + (c - Cx)) * HW;
            const f4 r = load4(reset_pre + hp, i, HW, vec), hv = load4(h + hp, i, HW, vec);
#pragma unroll
            for (int k = 0; k < 4; ++k) o.v[k] = hv.v[k] * sig2(r.v[k]).s;
        } else {
            o = zero4();
        }
        store4(out + plane * HW, i, HW, vec, o);
    }
}

// items as the forward's.  grad_x = grad_out[:, :Cx]; grad_reset_pre = g h r (1 - r); grad_h = grad_h_in + g r
__global__ __launch_bounds__(kThreads) void gru_reset_bwd_kernel(const float *__restrict__ grad_out, const float *__restrict__ reset_pre,
                                                                 const float *__restrict__ h, const float *__restrict__ grad_h_in,
                                                                 float *__restrict__ grad_x, float *__restrict__ grad_reset_pre,
                                                                 float *__restrict__ grad_h, int64_t B, int Cx, int C, int64_t HW,
                                                                 int vec) {
    const int Ct = Cx + C;
    const int64_t nq = (HW + 3) / 4, total = B * Ct * nq;
    for (int64_t id = (int64_t)blockIdx.x * kThreads + threadIdx.x; id < total; id += (int64_t)gridDim.x * kThreads) {
        const int64_t plane = id / nq, i = 4 * (id - plane * nq);
        const int64_t b = plane / Ct, c = plane - b * Ct;
        if (c < Cx) {
            if (grad_x) store4(grad_x + (b * Cx + c) * HW, i, HW, vec, load4(grad_out + plane * HW, i, HW, vec));
            continue;
        }
        const int64_t hp = (b * C + (c - Cx)) * HW;
        f4 dr = zero4(), dh = zero4();
        if (h) {
            const f4 g = load4(grad_out + plane * HW, i, HW, vec), rp = load4(reset_pre + hp, i, HW, vec), hv = load4(h + hp, i, HW, vec);
            const f4 acc = load4_opt(grad_h_in ? grad_h_in + hp : nullptr, i, HW, vec);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const Sig r = sig2(rp.v[k]);
                dr.v[k] = g.v[k] * hv.v[k] * (r.s * r.c);
                dh.v[k] = acc.v[k] + g.v[k] * r.s;
            }
        }
        store4(grad_reset_pre + hp, i, HW, vec, dr);
        if (grad_h) store4(grad_h + hp, i, HW, vec, dh);
    }
}

// items: B * C planes x quads
__global__ __launch_bounds__(kThreads) void gru_update_fwd_kernel(const float *__restrict__ update_pre, const float *__restrict__ out_pre,
                                                                  const float *__restrict__ h, float *__restrict__ new_state,
                                                                  int64_t planes, int64_t HW, int vec) {
    const int64_t nq = (HW + 3) / 4, total = planes * nq;
    for (int64_t id = (int64_t)blockIdx.x * kThreads + threadIdx.x; id < total; id += (int64_t)gridDim.x * kThreads) {
        const int64_t plane = id / nq, i = 4 * (id - plane * nq), p = plane * HW;
        const f4 up = load4(update_pre + p, i, HW, vec), op = load4(out_pre + p, i, HW, vec);
        const f4 hv = load4_opt(h ? h + p : nullptr, i, HW, vec);
        f4 n;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const Sig u = sig2(up.v[k]);
            n.v[k] = hv.v[k] * u.c + tanhf(op.v[k]) * u.s;
        }
        store4(new_state + p, i, HW, vec, n);
    }
}

__global__ __launch_bounds__(kThreads) void gru_update_bwd_kernel(const float *__restrict__ update_pre, const float *__restrict__ out_pre,
                                                                  const float *__restrict__ h, const float *__restrict__ grad_new,
                                                                  float *__restrict__ grad_update_pre, float *__restrict__ grad_out_pre,
                                                                  float *__restrict__ grad_h, int64_t planes, int64_t HW, int vec) {
    const int64_t nq = (HW + 3) / 4, total = planes * nq;
    for (int64_t id = (int64_t)blockIdx.x * kThreads + threadIdx.x; id < total; id += (int64_t)gridDim.x * kThreads) {
        const int64_t plane = id / nq, i = 4 * (id - plane * nq), p = plane * HW;
        const f4 up = load4(update_pre + p, i, HW, vec), op = load4(out_pre + p, i, HW, vec), g = load4(grad_new + p, i, HW, vec);
        const f4 hv = load4_opt(h ? h + p : nullptr, i, HW, vec);
        f4 du, dop, dh;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const Sig u = sig2(up.v[k]);
            const float t = tanhf(op.v[k]);
            du.v[k] = g.v[k] * (t - hv.v[k]) * (u.s * u.c);
            dop.v[k] = g.v[k] * u.s * sech2(op.v[k], t);
            dh.v[k] = g.v[k] * u.c;
        }
        store4(grad_update_pre + p, i, HW, vec, du);
        store4(grad_out_pre + p, i, HW, vec, dop);
        if (grad_h) store4(grad_h + p, i, HW, vec, dh);
    }
}

// ---------------------------------------------------------------------------------------------- bilinear up-sampling
// Output coordinate o of an axis of n source pixels, scale S, align_corners = False: source coordinate (o + 0.5) / S - 0.5, a
// negative one clamped to 0; i0 = its integer part, i1 = i0 + 1 below n - 1 (else i0), l1 = the fraction, l0 = 1 - l1.
struct Tap {
    int i0, i1;
    float l0, l1;
};

template <int S>
__device__ inline Tap tap_of(int o, int n) {
    float src = ((float)o + 0.5f) * (1.f / (float)S) - 0.5f;
    src = src < 0.f ? 0.f : src;
    Tap t;
    t.i0 = min((int)src, n - 1);
    t.i1 = t.i0 < n - 1 ? t.i0 + 1 : t.i0;
    t.l1 = src - (float)t.i0;
    t.l0 = 1.f - t.l1;
    return t;
}

// items: planes * Ho rows x ceil(Wo / 4) quads; a lane owns outputs (plane, yo, 4 q .. 4 q + 3)
template <int S>
__global__ __launch_bounds__(kThreads) void bilinear_up_fwd_kernel(const float *__restrict__ x, float *__restrict__ out, int64_t planes,
                                                                   int H, int W, int vec) {
    const int Ho = S * H, Wo = S * W;
    const int64_t nq = (Wo + 3) / 4, total = planes * Ho * nq;
    for (int64_t id = (int64_t)blockIdx.x * kThreads + threadIdx.x; id < total; id += (int64_t)gridDim.x * kThreads) {
        const int64_t row = id / nq;                     // plane * Ho + yo
        const int q = (int)(id - row * nq);
        const int64_t plane = row / Ho;
        const int yo = (int)(row - plane * Ho);
        const Tap ty = tap_of<S>(yo, H);
        const float *r0 = x + (plane * H + ty.i0) * W, *r1 = x + (plane * H + ty.i1) * W;
        f4 o;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int xo = 4 * q + k;
            float v = 0.f;
            if (xo < Wo) {
                const Tap tx = tap_of<S>(xo, W);
                v = ty.l0 * (tx.l0 * r0[tx.i0] + tx.l1 * r0[tx.i1]) + ty.l1 * (tx.l0 * r1[tx.i0] + tx.l1 * r1[tx.i1]);
            }
            o.v[k] = v;
        }
        store4(out + row * Wo, 4 * q, Wo, vec != 0, o);
    }
}

// weight of source index `i` in output coordinate o (both taps may name it: the last pixel of an axis)
template <int S>
__device__ inline float weight_of(int o, int i, int n) {
    const Tap t = tap_of<S>(o, n);
    return (t.i0 == i ? t.l0 : 0.f) + (t.i1 == i ? t.l1 : 0.f);
}

// one thread per INPUT pixel: its contributors are the outputs o in [S i - S / 2, S i + 3 S / 2 - 1] of each axis (inside the
// map), added row by row, left to right
template <int S>
__global__ __launch_bounds__(kThreads) void bilinear_up_bwd_kernel(const float *__restrict__ grad_out, float *__restrict__ grad_x,
                                                                   int64_t planes, int H, int W) {
    const int Ho = S * H, Wo = S * W;
    const int64_t total = planes * H * W;
    for (int64_t id = (int64_t)blockIdx.x * kThreads + threadIdx.x; id < total; id += (int64_t)gridDim.x * kThreads) {
        const int64_t rowi = id / W;                     // plane * H + iy
        const int ix = (int)(id - rowi * W);
        const int64_t plane = rowi / H;
        const int iy = (int)(rowi - plane * H);
        const int ox0 = S * ix - S / 2, oy0 = S * iy - S / 2;
        float wx[2 * S];
#pragma unroll
        for (int k = 0; k < 2 * S; ++k) {
            const int ox = ox0 + k;
            wx[k] = ox >= 0 && ox < Wo ? weight_of<S>(ox, ix, W) : 0.f;
        }
        const float *g = grad_out + plane * Ho * Wo;
        float acc = 0.f;
#pragma unroll
        for (int j = 0; j < 2 * S; ++j) {
            const int oy = oy0 + j;
            if (oy < 0 || oy >= Ho) continue;
            const float wy = weight_of<S>(oy, iy, H);
            const float *gr = g + (int64_t)oy * Wo;
#pragma unroll
            for (int k = 0; k < 2 * S; ++k) {
                const int ox = ox0 + k;
                if (ox >= 0 && ox < Wo) acc = acc + (wy * wx[k]) * gr[ox];
            }
        }
        grad_x[id] = acc;
    }
}

int check_cell(const char *what, int64_t B, int64_t C, int64_t HW) {
    if (B < 1 || C < 1 || HW < 1) return fail(EBFI_ERR_ARG, "%s: B = %lld, C = %lld, H * W = %lld must be positive", what, (long long)B, (long long)C, (long long)HW);
    if (C >= ((int64_t)1 << 28) || HW >= ((int64_t)1 << 40) || B * C >= ((int64_t)1 << 40) / 4 || B * C * 4 * HW >= ((int64_t)1 << 60))
        return fail(EBFI_ERR_ARG, "%s: B = %lld, C = %lld, H * W = %lld is too large", what, (long long)B, (long long)C, (long long)HW);
    return EBFI_OK;
}

unsigned grid_for(int64_t items) {
    const int64_t blocks = ceil_div(items, kThreads);
    return (unsigned)(blocks < kMaxBlocks ? blocks : kMaxBlocks);
}

bool all_aligned(std::initializer_list<const void *> ps) {
    for (const void *p : ps)
        if (p && !aligned16(p)) return false;
    return true;
}

}  // namespace

extern "C" int ebfi_lstm_cell_forward(const float *gates, const float *prev_cell, float *hidden, float *cell, int64_t B, int C, int64_t HW,
                                      void *stream) {
    if (!gates || !hidden || !cell) return fail(EBFI_ERR_ARG, "lstm_cell_forward: null pointer");
    if (int rc = check_cell("lstm_cell_forward", B, C, HW)) return rc;
    const int vec = HW % 4 == 0 && all_aligned({gates, prev_cell, hidden, cell});
    hipStream_t st = static_cast<hipStream_t>(stream);
    {
        ProfScope ps_("lstm_cell_fwd", st, 0.0, (prev_cell ? 7.0 : 6.0) * 4.0 * (double)B * C * (double)HW);
        hipLaunchKernelGGL(lstm_cell_fwd_kernel, dim3(grid_for(B * C * ceil_div(HW, 4))), dim3(kThreads), 0, st, gates, prev_cell, hidden,
                           cell, B * C, C, HW, vec);
    }
    return check_launch("lstm_cell_forward");
}

extern "C" int ebfi_lstm_cell_backward(const float *gates, const float *prev_cell, const float *cell, const float *grad_hidden,
                                       const float *grad_cell, float *grad_gates, float *grad_prev_cell, int64_t B, int C, int64_t HW,
                                       void *stream) {
    if (!gates || !cell || !grad_gates) return fail(EBFI_ERR_ARG, "lstm_cell_backward: null pointer");
    if (int rc = check_cell("lstm_cell_backward", B, C, HW)) return rc;
    const int vec = HW % 4 == 0 && all_aligned({gates, prev_cell, cell, grad_hidden, grad_cell, grad_gates, grad_prev_cell});
    hipStream_t st = static_cast<hipStream_t>(stream);
    {
        const double planes = 9.0 + (prev_cell ? 1.0 : 0.0) + (grad_hidden ? 1.0 : 0.0) + (grad_cell ? 1.0 : 0.0) + (grad_prev_cell ? 1.0 : 0.0);
        ProfScope ps_("lstm_cell_bwd", st, 0.0, planes * 4.0 * (double)B * C * (double)HW);
        hipLaunchKernelGGL(lstm_cell_bwd_kernel, dim3(grid_for(B * C * ceil_div(HW, 4))), dim3(kThreads), 0, st, gates, prev_cell, cell,
                           grad_hidden, grad_cell, grad_gates, grad_prev_cell, B * C, C, HW, vec);
    }
    return check_launch("lstm_cell_backward");
}

extern "C" int ebfi_gru_reset_forward(const float *reset_pre, const float *x, const float *h, float *out, int64_t B, int Cx, int C,
                                      int64_t HW, void *stream) {
    if (!reset_pre || !x || !out) return fail(EBFI_ERR_ARG, "gru_reset_forward: null pointer");
    if (Cx < 1) return fail(EBFI_ERR_ARG, "gru_reset_forward: Cx = %d must be positive", Cx);
    if (int rc = check_cell("gru_reset_forward", B, (int64_t)Cx + C, HW)) return rc;
    if (int rc = check_cell("gru_reset_forward", B, C, HW)) return rc;
    const int vec = HW % 4 == 0 && all_aligned({reset_pre, x, h, out});
    hipStream_t st = static_cast<hipStream_t>(stream);
    {
        ProfScope ps_("gru_reset_fwd", st, 0.0, (2.0 * Cx + (h ? 3.0 : 1.0) * C) * 4.0 * (double)B * (double)HW);
        hipLaunchKernelGGL(gru_reset_fwd_kernel, dim3(grid_for(B * (Cx + C) * ceil_div(HW, 4))), dim3(kThreads), 0, st, reset_pre, x, h, out,
                           B, Cx, C, HW, vec);
    }
    return check_launch("gru_reset_forward");
}

extern "C" int ebfi_gru_reset_backward(const float *grad_out, const float *reset_pre, const float *h, const float *grad_h_in, float *grad_x,
                                       float *grad_reset_pre, float *grad_h, int64_t B, int Cx, int C, int64_t HW, void *stream) {
    if (!grad_out || !reset_pre || !grad_reset_pre) return fail(EBFI_ERR_ARG, "gru_reset_backward: null pointer");
    if (Cx < 1) return fail(EBFI_ERR_ARG, "gru_reset_backward: Cx = %d must be positive", Cx);
    if (int rc = check_cell("gru_reset_backward", B, (int64_t)Cx + C, HW)) return rc;
    if (int rc = check_cell("gru_reset_backward", B, C, HW)) return rc;
    const int vec = HW % 4 == 0 && all_aligned({grad_out, reset_pre, h, grad_h_in, grad_x, grad_reset_pre, grad_h});
    hipStream_t st = static_cast<hipStream_t>(stream);
    {
        ProfScope ps_("gru_reset_bwd", st, 0.0, (2.0 * Cx + 5.0 * C) * 4.0 * (double)B * (double)HW);
        hipLaunchKernelGGL(gru_reset_bwd_kernel, dim3(grid_for(B * (Cx + C) * ceil_div(HW, 4))), dim3(kThreads), 0, st, grad_out, reset_pre, h,
                           grad_h_in, grad_x, grad_reset_pre, grad_h, B, Cx, C, HW, vec);
    }
    return check_launch("gru_reset_backward");
}

extern "C" int ebfi_gru_update_forward(const float *update_pre, const float *out_pre, const float *h, float *new_state, int64_t B, int C,
                                       int64_t HW, void *stream) {
    if (!update_pre || !out_pre || !new_state) return fail(EBFI_ERR_ARG, "gru_update_forward: null pointer");
    if (int rc = check_cell("gru_update_forward", B, C, HW)) return rc;
    const int vec = HW % 4 == 0 && all_aligned({update_pre, out_pre, h, new_state});
    hipStream_t st = static_cast<hipStream_t>(stream);
    {
        ProfScope ps_("gru_update_fwd", st, 0.0, (h ? 4.0 : 3.0) * 4.0 * (double)B * C * (double)HW);
        hipLaunchKernelGGL(gru_update_fwd_kernel, dim3(grid_for(B * C * ceil_div(HW, 4))), dim3(kThreads), 0, st, update_pre, out_pre, h,
                           new_state, B * C, HW, vec);
    }
    return check_launch("gru_update_forward");
}

extern "C" int ebfi_gru_update_backward(const float *update_pre, const float *out_pre, const float *h, const float *grad_new,
                                        float *grad_update_pre, float *grad_out_pre, float *grad_h, int64_t B, int C, int64_t HW,
                                        void *stream) {
    if (!update_pre || !out_pre || !grad_new || !grad_update_pre || !grad_out_pre) return fail(EBFI_ERR_ARG, "gru_update_backward: null pointer");
    if (int rc = check_cell("gru_update_backward", B, C, HW)) return rc;
    const int vec = HW % 4 == 0 && all_aligned({update_pre, out_pre, h, grad_new, grad_update_pre, grad_out_pre, grad_h});
    hipStream_t st = static_cast<hipStream_t>(stream);
    {
        ProfScope ps_("gru_update_bwd", st, 0.0, (5.0 + (h ? 1.0 : 0.0) + (grad_h ? 1.0 : 0.0)) * 4.0 * (double)B * C * (double)HW);
        hipLaunchKernelGGL(gru_update_bwd_kernel, dim3(grid_for(B * C * ceil_div(HW, 4))), dim3(kThreads), 0, st, update_pre, out_pre, h,
                           grad_new, grad_update_pre, grad_out_pre, grad_h, B * C, HW, vec);
    }
    return check_launch("gru_update_backward");
}

namespace {
int check_up(const char *what, int64_t planes, int H, int W, int scale) {
    if (scale != 2 && scale != 4) return fail(EBFI_ERR_ARG, "%s: scale = %d is not 2 or 4", what, scale);
    if (planes < 1 || H < 1 || W < 1) return fail(EBFI_ERR_ARG, "%s: planes = %lld, H = %d, W = %d must be positive", what, (long long)planes, H, W);
    if ((int64_t)scale * H >= ((int64_t)1 << 30) || (int64_t)scale * W >= ((int64_t)1 << 30) || planes >= ((int64_t)1 << 40) ||
        (double)planes * scale * scale * (double)H * (double)W >= 9e18)
        return fail(EBFI_ERR_ARG, "%s: planes = %lld, H = %d, W = %d at scale %d is too large", what, (long long)planes, H, W, scale);
    return EBFI_OK;
}
}  // namespace

extern "C" int ebfi_bilinear_up_forward(const float *x, float *out, int64_t planes, int H, int W, int scale, void *stream) {
    if (!x || !out) return fail(EBFI_ERR_ARG, "bilinear_up_forward: null pointer");
    if (int rc = check_up("bilinear_up_forward", planes, H, W, scale)) return rc;
    const int vec = ((int64_t)scale * W) % 4 == 0 && aligned16(out);
    const int64_t items = planes * scale * H * ceil_div((int64_t)scale * W, 4);
    hipStream_t st = static_cast<hipStream_t>(stream);
    {
        ProfScope ps_("bilinear_up_fwd", st, 0.0, (1.0 + scale * scale) * 4.0 * (double)planes * H * (double)W);
        if (scale == 2)
            hipLaunchKernelGGL(bilinear_up_fwd_kernel<2>, dim3(grid_for(items)), dim3(kThreads), 0, st, x, out, planes, H, W, vec);
        else
            hipLaunchKernelGGL(bilinear_up_fwd_kernel<4>, dim3(grid_for(items)), dim3(kThreads), 0, st, x, out, planes, H, W, vec);
    }
    return check_launch("bilinear_up_forward");
}

extern "C" int ebfi_bilinear_up_backward(const float *grad_out, float *grad_x, int64_t planes, int H, int W, int scale, void *stream) {
    if (!grad_out || !grad_x) return fail(EBFI_ERR_ARG, "bilinear_up_backward: null pointer");
    if (int rc = check_up("bilinear_up_backward", planes, H, W, scale)) return rc;
    const int64_t items = planes * H * W;
    hipStream_t st = static_cast<hipStream_t>(stream);
    {
        ProfScope ps_("bilinear_up_bwd", st, 0.0, (1.0 + scale * scale) * 4.0 * (double)planes * H * (double)W);
        if (scale == 2)
            hipLaunchKernelGGL(bilinear_up_bwd_kernel<2>, dim3(grid_for(items)), dim3(kThreads), 0, st, grad_out, grad_x, planes, H, W);
        else
            hipLaunchKernelGGL(bilinear_up_bwd_kernel<4>, dim3(grid_for(items)), dim3(kThreads), 0, st, grad_out, grad_x, planes, H, W);
    }
    return check_launch("bilinear_up_backward");
}
