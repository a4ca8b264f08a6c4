// Adam update of the training step (train_ours.py:276-277: optimizer.step() of torch.optim.Adam, config train_ours.yml
// :59-65) over the ONE flat parameter buffer the engine trains (ebfi_amd.dp.FlatAdam): 5.7 M elements in one pass of
// 16-byte accesses.  PyTorch's fused multi-tensor kernel walks a single tensor in 64 K-element chunks -- 87 workgroups
// for this model, 112 us; this launch is bandwidth-bound (7 maps of 22.8 MB).
// Arithmetic follows torch's fused Adam: m <- m + (1-b1)(g - m); v <- b2 v + (1-b2) g^2; bias corrections 1 - b^t in
// double precision; p <- p - (lr / c1) m / (sqrt(v) / sqrt(c2) + eps).
#include "common.hpp"

using namespace ebfi;

namespace {

__global__ __launch_bounds__(256) void adam_flat_kernel(float *__restrict__ p, const float *__restrict__ g, float *__restrict__ m,
                                                        float *__restrict__ v, float *__restrict__ step, int64_t n4,
                                                        int64_t n, double lr, double beta1, double beta2, double eps,
                                                        int *__restrict__ guard, const float *__restrict__ flag) {
    // guard (optional): guard[0] != 0 marks this step's gradient as unusable (an fp16 operand of the backward pass left its
    // range, conv2d_f16.inc.hpp): nothing is updated, the step count is taken back, guard[1] counts the skipped steps.
    // flag (optional, with guard): the ranks' guard flags summed by the gradient all-reduce (ebfi_grad_gather put this rank's
    // into the wire buffer); anything but an exact zero skips the step on every rank and is written back to guard[0].
    // (Every thread reads the same two words; thread 0 of block 0 is the only writer and writes only values that keep the
    // other threads' decision: guard[0] becomes non-zero only when the flag already said "skip".)
    if (guard != nullptr) {
        const bool by_flag = flag != nullptr && !(flag[0] == 0.f);
        if (guard[0] != 0 || by_flag) {
            if (blockIdx.x == 0 && threadIdx.x == 0) {
                step[0] -= 1.f;
                guard[1] += 1;
                if (by_flag) guard[0] = 1;
            }
            return;
        }
    }
    const double t = (double)step[0];
    const double c1 = 1.0 - pow(beta1, t), c2 = 1.0 - pow(beta2, t);
    const float step_size = (float)(lr / c1), c2s = (float)sqrt(c2);
    const float w1 = (float)(1.0 - beta1), b2 = (float)beta2, w2 = (float)(1.0 - beta2), e = (float)eps;
    auto upd = [&](float &pp, float gg, float &mm, float &vv) {
        mm = mm + w1 * (gg - mm);
        vv = b2 * vv + w2 * gg * gg;
        const float denom = sqrtf(vv) / c2s + e;
        pp -= step_size * mm / denom;
    };
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n4) {
        float4 P = reinterpret_cast<float4 *>(p)[i], M = reinterpret_cast<float4 *>(m)[i], V = reinterpret_cast<float4 *>(v)[i];
        const float4 G = reinterpret_cast<const float4 *>(g)[i];
        upd(P.x, G.x, M.x, V.x);
        upd(P.y, G.y, M.y, V.y);
        upd(P.z, G.z, M.z, V.z);
        upd(P.w, G.w, M.w, V.w);
        reinterpret_cast<float4 *>(p)[i] = P;
        reinterpret_cast<float4 *>(m)[i] = M;
        reinterpret_cast<float4 *>(v)[i] = V;
    }
    if (i == 0)
        for (int64_t k = n4 * 4; k < n; ++k) upd(p[k], g[k], m[k], v[k]);
}

// The optimiser section of the config beyond plain Adam (ebfi_amd.dp.FlatOptimizer; the reference builds its optimiser with
// eval(config['optimizer']['name'])(params, **config['optimizer']['args']), train_ours.py:770-771): Adam / AdamW with weight
// decay and AMSGrad, and SGD with weight decay, momentum, dampening and Nesterov, each as ONE launch over the flat buffer with
// the guard protocol of adam_flat_kernel.  Every option is a template parameter, so a variant loads and stores only the maps
// it needs: plain SGD 3 (p read + written, g read), SGD with momentum 5, Adam 7, AMSGrad 9.  `g` is only read: weight decay is
// added in registers, never into the gradient buffer (the all-reduce's wire buffer, which telemetry reads after the step).
// The arithmetic is torch's single-tensor step operation by operation, with the roundings of its float32 CPU kernels spelled
// out (contraction off, an explicit fma exactly where add(alpha=) / lerp / addcmul fuse):
//   Adam   g' = fma(p, wd, g) (L2)  |  p <- p (1 - lr wd) (decoupled);  m <- fma(1-b1, g' - m, m);
//          v <- fma((1-b2) g', g', b2 v);  vmax <- max(vmax, v);  p <- p - (lr/c1 m) / (sqrt(v | vmax) / sqrt(c2) + eps)
//   SGD    d = fma(p, wd, g);  buf <- d on the first applied step, fma(d, 1-dampening, momentum buf) afterwards;
//          d <- fma(buf, momentum, d) (Nesterov) | buf;  p <- fma(d, -lr, p)
// "First applied step" is step[0] == 1 on the device: the host increments the word before the launch and a skipped step
// takes it back, so a first step skipped by the overflow guard leaves the next one the first.
enum { WD_NONE = 0, WD_L2 = 1, WD_DECOUPLED = 2 };
enum { MOM_NONE = 0, MOM_PLAIN = 1, MOM_NESTEROV = 2 };

struct OptimArgs {
    double lr, beta1, beta2, eps, weight_decay, momentum, dampening;
};

struct AdamCoef {
    float step_size, c2s, w1, b2, w2, eps, wd, keep;
};

template <int WD, bool AMS>
__device__ __forceinline__ void adam_elem(float &pp, float gg, float &mm, float &vv, float &xx, const AdamCoef &c) {
#pragma clang fp contract(off)
    if (WD == WD_L2) gg = __builtin_fmaf(pp, c.wd, gg);
    if (WD == WD_DECOUPLED) pp = pp * c.keep;
    mm = __builtin_fmaf(c.w1, gg - mm, mm);
    vv = __builtin_fmaf(c.w2 * gg, gg, vv * c.b2);
    float s = vv;
    if (AMS) {
        xx = (xx != xx || xx >= vv) ? xx : vv;          // torch.maximum: a NaN on either side stays
        s = xx;
    }
    const float denom = sqrtf(s) / c.c2s + c.eps;
    pp = pp - (c.step_size * mm) / denom;
}

struct SgdCoef {
    float neg_lr, wd, mom, undamp;
    bool first;
};

template <int WD, int MOM>
__device__ __forceinline__ void sgd_elem(float &pp, float gg, float &bb, const SgdCoef &c) {
#pragma clang fp contract(off)
    float d = gg;
    if (WD == WD_L2) d = __builtin_fmaf(pp, c.wd, gg);
    if (MOM != MOM_NONE) {
        bb = c.first ? d : __builtin_fmaf(d, c.undamp, bb * c.mom);
        d = MOM == MOM_NESTEROV ? __builtin_fmaf(bb, c.mom, d) : bb;
    }
    pp = __builtin_fmaf(d, c.neg_lr, pp);
}

// guard / flag: the protocol of adam_flat_kernel, word for word (plain SGD has no step word: nothing to take back there)
__device__ __forceinline__ bool optim_skipped(float *__restrict__ step, int *__restrict__ guard, const float *__restrict__ flag) {
    if (guard != nullptr) {
        const bool by_flag = flag != nullptr && !(flag[0] == 0.f);
        if (guard[0] != 0 || by_flag) {
            if (blockIdx.x == 0 && threadIdx.x == 0) {
                if (step != nullptr) step[0] -= 1.f;
                guard[1] += 1;
                if (by_flag) guard[0] = 1;
            }
            return true;
        }
    }
    return false;
}

template <int WD, bool AMS>
__global__ __launch_bounds__(256) void adam_opt_kernel(float *__restrict__ p, const float *__restrict__ g, float *__restrict__ m,
                                                       float *__restrict__ v, float *__restrict__ vmax, float *__restrict__ step,
                                                       int64_t n4, int64_t n, OptimArgs a, int *__restrict__ guard,
                                                       const float *__restrict__ flag) {
    if (optim_skipped(step, guard, flag)) return;
    const double t = (double)step[0];
    const double c1 = 1.0 - pow(a.beta1, t), c2 = 1.0 - pow(a.beta2, t);
    AdamCoef c;
    c.step_size = (float)(a.lr / c1), c.c2s = (float)sqrt(c2);
    c.w1 = (float)(1.0 - a.beta1), c.b2 = (float)a.beta2, c.w2 = (float)(1.0 - a.beta2), c.eps = (float)a.eps;
    c.wd = (float)a.weight_decay, c.keep = (float)(1.0 - a.lr * a.weight_decay);
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n4) {
        float4 P = reinterpret_cast<float4 *>(p)[i], M = reinterpret_cast<float4 *>(m)[i], V = reinterpret_cast<float4 *>(v)[i];
        const float4 G = reinterpret_cast<const float4 *>(g)[i];
        float4 X = make_float4(0.f, 0.f, 0.f, 0.f);
        if (AMS) X = reinterpret_cast<float4 *>(vmax)[i];
        adam_elem<WD, AMS>(P.x, G.x, M.x, V.x, X.x, c);
        adam_elem<WD, AMS>(P.y, G.y, M.y, V.y, X.y, c);
        adam_elem<WD, AMS>(P.z, G.z, M.z, V.z, X.z, c);
        adam_elem<WD, AMS>(P.w, G.w, M.w, V.w, X.w, c);
        reinterpret_cast<float4 *>(p)[i] = P;
        reinterpret_cast<float4 *>(m)[i] = M;
        reinterpret_cast<float4 *>(v)[i] = V;
        if (AMS) reinterpret_cast<float4 *>(vmax)[i] = X;
    }
    if (i == 0)
        for (int64_t k = n4 * 4; k < n; ++k) {
            float x = 0.f;
            if (AMS) x = vmax[k];
            adam_elem<WD, AMS>(p[k], g[k], m[k], v[k], x, c);
            if (AMS) vmax[k] = x;
        }
}

template <int WD, int MOM>
__global__ __launch_bounds__(256) void sgd_opt_kernel(float *__restrict__ p, const float *__restrict__ g, float *__restrict__ buf,
                                                      float *__restrict__ step, int64_t n4, int64_t n, OptimArgs a,
                                                      int *__restrict__ guard, const float *__restrict__ flag) {
    if (optim_skipped(step, guard, flag)) return;
    SgdCoef c;
    c.neg_lr = (float)(-a.lr), c.wd = (float)a.weight_decay, c.mom = (float)a.momentum, c.undamp = (float)(1.0 - a.dampening);
    c.first = MOM != MOM_NONE && step[0] == 1.f;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n4) {
        float4 P = reinterpret_cast<float4 *>(p)[i];
        const float4 G = reinterpret_cast<const float4 *>(g)[i];
        float4 B = make_float4(0.f, 0.f, 0.f, 0.f);
        if (MOM != MOM_NONE) B = reinterpret_cast<float4 *>(buf)[i];
        sgd_elem<WD, MOM>(P.x, G.x, B.x, c);
        sgd_elem<WD, MOM>(P.y, G.y, B.y, c);
        sgd_elem<WD, MOM>(P.z, G.z, B.z, c);
        sgd_elem<WD, MOM>(P.w, G.w, B.w, c);
        reinterpret_cast<float4 *>(p)[i] = P;
        if (MOM != MOM_NONE) reinterpret_cast<float4 *>(buf)[i] = B;
    }
    if (i == 0)
        for (int64_t k = n4 * 4; k < n; ++k) {
            float b = 0.f;
            if (MOM != MOM_NONE) b = buf[k];
            sgd_elem<WD, MOM>(p[k], g[k], b, c);
            if (MOM != MOM_NONE) buf[k] = b;
        }
}

// ebfi_optim_step_ex: the same laws with a gradient scale (the clipping coefficient ebfi_grad_norm left on the device) in front
// and an exponential moving average of the parameters behind, still ONE launch: the scale costs no map (one word, `g` stays
// read-only: the scaled gradient lives in registers only), the average two (e read + written).  Continuing the list above,
// contraction off:
//   g' = g * s  (s = grad_scale[0], or 1 without one: x * 1 is x, bit for bit) BEFORE the L2 fma, as clipping precedes
//   the optimiser in torch;  <the update above on g'>;  e <- e + w * (p_new - e),  w = (float)(1 - d),
//   d = ema_decay | min(ema_decay, (1 + t) / (10 + t)) (warm-up), t = ema_step[0] in double
// adam_elem / sgd_elem are the functions the kernels above inline, so a scale s gives the bits ebfi_optim_step gives on a
// gradient multiplied by s in float32 beforehand.  The guard protocol is optim_skipped's, word for word, extended to the
// average: a skipped step takes ema_step back too, writes no e, and counts once in guard[1].
struct EmaArgs {
    double decay;
    int warmup;
};

__device__ __forceinline__ float scaled(float gg, float s) {
#pragma clang fp contract(off)
    return gg * s;
}

__device__ __forceinline__ void ema_elem(float &ee, float pp, float w) {
#pragma clang fp contract(off)
    const float d = pp - ee;
    ee = ee + w * d;
}

__device__ __forceinline__ float ema_weight(const float *__restrict__ ema_step, const EmaArgs &ea) {
    double d = ea.decay;
    if (ea.warmup) {
        const double t = (double)ema_step[0];
        const double ramp = (1.0 + t) / (10.0 + t);
        d = ramp < d ? ramp : d;
    }
    return (float)(1.0 - d);
}

__device__ __forceinline__ bool optim_skipped_ex(float *__restrict__ step, float *__restrict__ ema_step, int *__restrict__ guard,
                                                 const float *__restrict__ flag) {
    if (guard != nullptr) {
        const bool by_flag = flag != nullptr && !(flag[0] == 0.f);
        if (guard[0] != 0 || by_flag) {
            if (blockIdx.x == 0 && threadIdx.x == 0) {
                if (step != nullptr) step[0] -= 1.f;
                if (ema_step != nullptr) ema_step[0] -= 1.f;
                guard[1] += 1;
                if (by_flag) guard[0] = 1;
            }
            return true;
        }
    }
    return false;
}

template <int WD, bool AMS, bool EMA>
__global__ __launch_bounds__(256) void adam_ex_kernel(float *__restrict__ p, const float *__restrict__ g, float *__restrict__ m,
                                                      float *__restrict__ v, float *__restrict__ vmax, float *__restrict__ step,
                                                      int64_t n4, int64_t n, OptimArgs a, int *__restrict__ guard,
                                                      const float *__restrict__ flag, const float *__restrict__ grad_scale,
                                                      float *__restrict__ ema, float *__restrict__ ema_step, EmaArgs ea) {
    if (optim_skipped_ex(step, EMA ? ema_step : nullptr, guard, flag)) return;
    const double t = (double)step[0];
    const double c1 = 1.0 - pow(a.beta1, t), c2 = 1.0 - pow(a.beta2, t);
    AdamCoef c;
    c.step_size = (float)(a.lr / c1), c.c2s = (float)sqrt(c2);
    c.w1 = (float)(1.0 - a.beta1), c.b2 = (float)a.beta2, c.w2 = (float)(1.0 - a.beta2), c.eps = (float)a.eps;
    c.wd = (float)a.weight_decay, c.keep = (float)(1.0 - a.lr * a.weight_decay);
    const float s = grad_scale != nullptr ? grad_scale[0] : 1.f;
    const float w = EMA ? ema_weight(ema_step, ea) : 0.f;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n4) {
        float4 P = reinterpret_cast<float4 *>(p)[i], M = reinterpret_cast<float4 *>(m)[i], V = reinterpret_cast<float4 *>(v)[i];
        const float4 G = reinterpret_cast<const float4 *>(g)[i];
        float4 X = make_float4(0.f, 0.f, 0.f, 0.f), E = make_float4(0.f, 0.f, 0.f, 0.f);
        if (AMS) X = reinterpret_cast<float4 *>(vmax)[i];
        if (EMA) E = reinterpret_cast<float4 *>(ema)[i];
        adam_elem<WD, AMS>(P.x, scaled(G.x, s), M.x, V.x, X.x, c);
        adam_elem<WD, AMS>(P.y, scaled(G.y, s), M.y, V.y, X.y, c);
        adam_elem<WD, AMS>(P.z, scaled(G.z, s), M.z, V.z, X.z, c);
        adam_elem<WD, AMS>(P.w, scaled(G.w, s), M.w, V.w, X.w, c);
        reinterpret_cast<float4 *>(p)[i] = P;
        reinterpret_cast<float4 *>(m)[i] = M;
        reinterpret_cast<float4 *>(v)[i] = V;
        if (AMS) reinterpret_cast<float4 *>(vmax)[i] = X;
        if (EMA) {
            ema_elem(E.x, P.x, w);
            ema_elem(E.y, P.y, w);
            ema_elem(E.z, P.z, w);
            ema_elem(E.w, P.w, w);
            reinterpret_cast<float4 *>(ema)[i] = E;
        }
    }
    if (i == 0)
        for (int64_t k = n4 * 4; k < n; ++k) {
            float x = 0.f;
            if (AMS) x = vmax[k];
            adam_elem<WD, AMS>(p[k], scaled(g[k], s), m[k], v[k], x, c);
            if (AMS) vmax[k] = x;
            if (EMA) ema_elem(ema[k], p[k], w);
        }
}

template <int WD, int MOM, bool EMA>
__global__ __launch_bounds__(256) void sgd_ex_kernel(float *__restrict__ p, const float *__restrict__ g, float *__restrict__ buf,
                                                     float *__restrict__ step, int64_t n4, int64_t n, OptimArgs a,
                                                     int *__restrict__ guard, const float *__restrict__ flag,
                                                     const float *__restrict__ grad_scale, float *__restrict__ ema,
                                                     float *__restrict__ ema_step, EmaArgs ea) {
    if (optim_skipped_ex(step, EMA ? ema_step : nullptr, guard, flag)) return;
    SgdCoef c;
    c.neg_lr = (float)(-a.lr), c.wd = (float)a.weight_decay, c.mom = (float)a.momentum, c.undamp = (float)(1.0 - a.dampening);
    c.first = MOM != MOM_NONE && step[0] == 1.f;
    const float s = grad_scale != nullptr ? grad_scale[0] : 1.f;
    const float w = EMA ? ema_weight(ema_step, ea) : 0.f;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n4) {
        float4 P = reinterpret_cast<float4 *>(p)[i];
        const float4 G = reinterpret_cast<const float4 *>(g)[i];
        float4 B = make_float4(0.f, 0.f, 0.f, 0.f), E = make_float4(0.f, 0.f, 0.f, 0.f);
        if (MOM != MOM_NONE) B = reinterpret_cast<float4 *>(buf)[i];
        if (EMA) E = reinterpret_cast<float4 *>(ema)[i];
        sgd_elem<WD, MOM>(P.x, scaled(G.x, s), B.x, c);
        sgd_elem<WD, MOM>(P.y, scaled(G.y, s), B.y, c);
        sgd_elem<WD, MOM>(P.z, scaled(G.z, s), B.z, c);
        sgd_elem<WD, MOM>(P.w, scaled(G.w, s), B.w, c);
        reinterpret_cast<float4 *>(p)[i] = P;
        if (MOM != MOM_NONE) reinterpret_cast<float4 *>(buf)[i] = B;
        if (EMA) {
            ema_elem(E.x, P.x, w);
            ema_elem(E.y, P.y, w);
            ema_elem(E.z, P.z, w);
            ema_elem(E.w, P.w, w);
            reinterpret_cast<float4 *>(ema)[i] = E;
        }
    }
    if (i == 0)
        for (int64_t k = n4 * 4; k < n; ++k) {
            float b = 0.f;
            if (MOM != MOM_NONE) b = buf[k];
            sgd_elem<WD, MOM>(p[k], scaled(g[k], s), b, c);
            if (MOM != MOM_NONE) buf[k] = b;
            if (EMA) ema_elem(ema[k], p[k], w);
        }
}

// Gradient packing of the training step (ebfi_amd.dp.FlatGradBucket.gather): the per-parameter gradient tensors autograd
// produced are copied into the one flat buffer the all-reduce and the Adam launch work on.  The source pointers travel BY VALUE
// in the kernel arguments, 128 tensors per launch (3 launches for the model's 255 parameters) -- nothing to upload, and a
// captured launch replays with the addresses its capture saw.  A tensor is cut into chunks of 16384 elements, one workgroup
// each (torch.cat's batched copy gives every input the same number of workgroups: the 1.8 M-element KernelConv weight next to
// 64-element biases took 90 us for the 22.8 MB); the workgroup finds its tensor by bisection over the chunk prefix sums.
// The last `pad` floats of the buffer carry this rank's overflow flag (guard[0] != 0) and zeros, so the flag travels inside the
// gradient message.
constexpr int GG_BATCH = 128, GG_CHUNK = 16384;
struct GatherBatch {
    const float *src[GG_BATCH];        // NULL: the parameter has no gradient, its range is zero-filled
    long long dst[GG_BATCH];           // element offset in the flat buffer
    int n[GG_BATCH];                   // elements
    unsigned chunk0[GG_BATCH + 1];     // prefix sums of ceil(n / GG_CHUNK); chunk0[count] = workgroups of this launch
    int count;
    int trailer;                       // 1: one extra workgroup writes the trailer
    unsigned chunks;                   // = chunk0[count] (a field of its own: no dynamic index into the kernarg table)
};

__global__ __launch_bounds__(256) void grad_gather_kernel(GatherBatch bt, float *__restrict__ flat, int64_t numel, int pad,
                                                          const int *__restrict__ guard) {
    const unsigned wg = blockIdx.x;
    if (wg == bt.chunks) {                          // (only when bt.trailer: the grid has one workgroup more)
        if ((int)threadIdx.x < pad) flat[numel + threadIdx.x] = (threadIdx.x == 0 && guard != nullptr && guard[0] != 0) ? 1.f : 0.f;
        return;
    }
    // this workgroup's tensor: the last k with chunk0[k] <= wg.  A linear walk with CONSTANT indices on purpose: the arguments
    // live in the kernarg segment, and a bisection's dynamic index made the compiler copy the table into scratch memory first
    // (144 bytes per lane); the walk is 128 scalar compare-and-select steps, uniform over the workgroup.
    const float *src = nullptr;
    long long dst0 = 0;
    int cnt = 0;
    unsigned c0 = 0;
#pragma unroll
    for (int k = 0; k < GG_BATCH; ++k) {
        if (k < bt.count && wg >= bt.chunk0[k]) {
            src = bt.src[k];
            dst0 = bt.dst[k];
            cnt = bt.n[k];
            c0 = bt.chunk0[k];
        }
    }
    const int o = (int)(wg - c0) * GG_CHUNK;
    const int n = min(GG_CHUNK, cnt - o);
    float *__restrict__ d = flat + dst0 + o;
    if (src == nullptr) {
        for (int i = threadIdx.x; i < n; i += 256) d[i] = 0.f;
        return;
    }
    const float *__restrict__ a = src + o;
    // 16-byte LOADS from the source as soon as it is 16-byte aligned (gradient tensors are: `sh` skips to the boundary), eight
    // of them in flight per thread; 16-byte STORES when the destination happens to share that alignment, four dword stores per
    // load otherwise -- parameter offsets are arbitrary element counts, and behind the first 3-element bias every destination
    // is misaligned: the first version fell back to a dword-per-iteration loop there (64 dependent round trips, 33 us per launch).
    typedef float f32x4 __attribute__((ext_vector_type(4)));
    const int sh = min(n, (int)((16u - ((unsigned)reinterpret_cast<uintptr_t>(a) & 15u)) & 15u) >> 2);
    if ((int)threadIdx.x < sh) d[threadIdx.x] = a[threadIdx.x];
    const int n4 = (n - sh) >> 2;
    const f32x4 *a4 = reinterpret_cast<const f32x4 *>(a + sh);
    float *dd = d + sh;
    const bool dst16 = (reinterpret_cast<uintptr_t>(dd) & 15u) == 0;
    for (int i0 = threadIdx.x; i0 < n4; i0 += 256 * 8) {
        f32x4 v[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) v[k] = a4[min(i0 + 256 * k, n4 - 1)];          // (unconditional, clamped: stays in registers)
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int i = i0 + 256 * k;
            if (i < n4) {
                if (dst16) {
                    reinterpret_cast<f32x4 *>(dd)[i] = v[k];
                } else {
                    dd[4 * i] = v[k].x; dd[4 * i + 1] = v[k].y; dd[4 * i + 2] = v[k].z; dd[4 * i + 3] = v[k].w;
                }
            }
        }
    }
    for (int i = sh + 4 * n4 + threadIdx.x; i < n; i += 256) d[i] = a[i];
}

}  // namespace

extern "C" int ebfi_grad_gather(const void *const *grads, const int64_t *numels, int count, float *flat, int64_t total, int pad,
                                const int *guard, void *stream) {
    if (!grads || !numels || !flat || count <= 0 || total <= 0 || pad < 1 || pad > 256) return fail(EBFI_ERR_ARG, "grad_gather: bad argument");
    int64_t sum = 0;
    for (int k = 0; k < count; ++k) {
        if (numels[k] < 0 || numels[k] > 0x7fffffff) return fail(EBFI_ERR_ARG, "grad_gather: tensor %d has %lld elements", k, (long long)numels[k]);
        if (grads[k] && (reinterpret_cast<uintptr_t>(grads[k]) & 3u)) return fail(EBFI_ERR_ARG, "grad_gather: tensor %d is not 4-byte aligned", k);
        sum += numels[k];
    }
    if (sum != total) return fail(EBFI_ERR_ARG, "grad_gather: the tensors hold %lld elements, the buffer %lld", (long long)sum, (long long)total);
    hipStream_t st = static_cast<hipStream_t>(stream);
    int64_t off = 0;
    for (int k0 = 0; k0 < count; k0 += GG_BATCH) {
        GatherBatch bt;
        bt.count = std::min(GG_BATCH, count - k0);
        bt.trailer = k0 + GG_BATCH >= count ? 1 : 0;
        unsigned chunks = 0;
        double bytes = 0.0;
        for (int j = 0; j < bt.count; ++j) {
            bt.src[j] = static_cast<const float *>(grads[k0 + j]);
            bt.dst[j] = off;
            bt.n[j] = (int)numels[k0 + j];
            bt.chunk0[j] = chunks;
            chunks += (unsigned)ceil_div(numels[k0 + j], (int64_t)GG_CHUNK);
            off += numels[k0 + j];
            bytes += 8.0 * (double)numels[k0 + j];
        }
        bt.chunk0[bt.count] = chunks;
        bt.chunks = chunks;
        for (int j = bt.count; j < GG_BATCH; ++j) bt.src[j] = nullptr, bt.dst[j] = 0, bt.n[j] = 0, bt.chunk0[j + 1] = chunks;
        if (chunks + (unsigned)bt.trailer == 0) continue;
        ProfScope ps("grad_gather", st, 0.0, bytes);
        hipLaunchKernelGGL(grad_gather_kernel, dim3(chunks + (unsigned)bt.trailer), dim3(256), 0, st, bt, flat, total, pad, guard);
    }
    return check_launch("grad_gather");
}

extern "C" int ebfi_adam_step_guarded(float *param, const float *grad, float *exp_avg, float *exp_avg_sq, float *step, int64_t n,
                                      double lr, double beta1, double beta2, double eps, int *guard, const float *flag, void *stream);

extern "C" int ebfi_adam_step(float *param, const float *grad, float *exp_avg, float *exp_avg_sq, const float *step, int64_t n,
                              double lr, double beta1, double beta2, double eps, void *stream) {
    return ebfi_adam_step_guarded(param, grad, exp_avg, exp_avg_sq, const_cast<float *>(step), n, lr, beta1, beta2, eps, nullptr, nullptr,
                                  stream);
}

extern "C" int ebfi_adam_step_guarded(float *param, const float *grad, float *exp_avg, float *exp_avg_sq, float *step, int64_t n,
                                      double lr, double beta1, double beta2, double eps, int *guard, const float *flag, void *stream) {
    if (flag && !guard) return fail(EBFI_ERR_ARG, "adam_step: an overflow flag needs the guard words");
    if (!param || !grad || !exp_avg || !exp_avg_sq || !step || n < 0) return fail(EBFI_ERR_ARG, "adam_step: null argument");
    if (!aligned16(param) || !aligned16(grad) || !aligned16(exp_avg) || !aligned16(exp_avg_sq))
        return fail(EBFI_ERR_ARG, "adam_step: buffers must be 16-byte aligned");
    if (n == 0) return EBFI_OK;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int64_t n4 = n / 4;
    {
        ProfScope ps("adam_flat", st, 0.0, 28.0 * (double)n);
        hipLaunchKernelGGL(adam_flat_kernel, dim3((unsigned)ceil_div(std::max<int64_t>(n4, 1), 256)), dim3(256), 0, st, param, grad,
                           exp_avg, exp_avg_sq, step, n4, n, lr, beta1, beta2, eps, guard, flag);
    }
    return check_launch("adam_flat");
}

namespace {

template <int WD, bool AMS>
void launch_adam_opt(const char *label, double maps, float *p, const float *g, float *m, float *v, float *vmax, float *step,
                     int64_t n, const OptimArgs &a, int *guard, const float *flag, hipStream_t st) {
    const int64_t n4 = n / 4;
    ProfScope ps(label, st, 0.0, maps * 4.0 * (double)n);
    hipLaunchKernelGGL((adam_opt_kernel<WD, AMS>), dim3((unsigned)ceil_div(std::max<int64_t>(n4, 1), 256)), dim3(256), 0, st, p, g,
                       m, v, vmax, step, n4, n, a, guard, flag);
}

template <int WD, int MOM>
void launch_sgd_opt(const char *label, double maps, float *p, const float *g, float *buf, float *step, int64_t n, const OptimArgs &a,
                    int *guard, const float *flag, hipStream_t st) {
    const int64_t n4 = n / 4;
    ProfScope ps(label, st, 0.0, maps * 4.0 * (double)n);
    hipLaunchKernelGGL((sgd_opt_kernel<WD, MOM>), dim3((unsigned)ceil_div(std::max<int64_t>(n4, 1), 256)), dim3(256), 0, st, p, g,
                       buf, step, n4, n, a, guard, flag);
}

}  // namespace

extern "C" int ebfi_optim_step(int kind, int flags, float *param, const float *grad, float *state0, float *state1, float *state2,
                               float *step, int64_t n, double lr, double beta1, double beta2, double eps, double weight_decay,
                               double momentum, double dampening, int *guard, const float *flag, void *stream) {
    if (kind != EBFI_OPTIM_ADAM && kind != EBFI_OPTIM_SGD)
        return fail(EBFI_ERR_UNSUPPORTED, "optim_step: unknown optimiser kind %d", kind);
    const int known = kind == EBFI_OPTIM_ADAM ? (EBFI_OPTIM_DECOUPLED_DECAY | EBFI_OPTIM_AMSGRAD) : EBFI_OPTIM_NESTEROV;
    if (flags & ~known) return fail(EBFI_ERR_ARG, "optim_step: option flags 0x%x do not belong to optimiser kind %d", flags, kind);
    if (!(weight_decay >= 0.0)) return fail(EBFI_ERR_ARG, "optim_step: weight_decay must not be negative");
    const bool ams = (flags & EBFI_OPTIM_AMSGRAD) != 0, decoupled = (flags & EBFI_OPTIM_DECOUPLED_DECAY) != 0;
    if (kind == EBFI_OPTIM_ADAM && !ams && weight_decay == 0.0)         // the default configuration: the launch it has always been
        return ebfi_adam_step_guarded(param, grad, state0, state1, step, n, lr, beta1, beta2, eps, guard, flag, stream);
    if (flag && !guard) return fail(EBFI_ERR_ARG, "optim_step: an overflow flag needs the guard words");
    if (!param || !grad || n < 0) return fail(EBFI_ERR_ARG, "optim_step: null argument");
    if (!aligned16(param) || !aligned16(grad)) return fail(EBFI_ERR_ARG, "optim_step: buffers must be 16-byte aligned");
    hipStream_t st = static_cast<hipStream_t>(stream);
    const OptimArgs a{lr, beta1, beta2, eps, weight_decay, momentum, dampening};
    if (kind == EBFI_OPTIM_ADAM) {
        if (!state0 || !state1 || !step || (ams && !state2))
            return fail(EBFI_ERR_ARG, "optim_step: Adam needs exp_avg, exp_avg_sq%s and the step word", ams ? ", max_exp_avg_sq" : "");
        if (!aligned16(state0) || !aligned16(state1) || (ams && !aligned16(state2)))
            return fail(EBFI_ERR_ARG, "optim_step: buffers must be 16-byte aligned");
        if (n == 0) return EBFI_OK;
        const int wd = weight_decay == 0.0 ? WD_NONE : decoupled ? WD_DECOUPLED : WD_L2;
        const double maps = ams ? 9.0 : 7.0;
#define EBFI_ADAM_CASE(W, A, L) \
    if (wd == W && ams == A) launch_adam_opt<W, A>(L, maps, param, grad, state0, state1, state2, step, n, a, guard, flag, st)
        EBFI_ADAM_CASE(WD_L2, false, "optim_adam_l2");
        EBFI_ADAM_CASE(WD_DECOUPLED, false, "optim_adamw");
        EBFI_ADAM_CASE(WD_NONE, true, "optim_adam_ams");
        EBFI_ADAM_CASE(WD_L2, true, "optim_adam_l2_ams");
        EBFI_ADAM_CASE(WD_DECOUPLED, true, "optim_adamw_ams");
#undef EBFI_ADAM_CASE
        return check_launch("optim_adam");
    }
    const bool nesterov = (flags & EBFI_OPTIM_NESTEROV) != 0;
    if (!(momentum >= 0.0)) return fail(EBFI_ERR_ARG, "optim_step: momentum must not be negative");
    if (nesterov && (momentum <= 0.0 || dampening != 0.0))
        return fail(EBFI_ERR_ARG, "optim_step: Nesterov momentum requires a momentum and zero dampening");
    const int mom = momentum == 0.0 ? MOM_NONE : nesterov ? MOM_NESTEROV : MOM_PLAIN;
    if (mom != MOM_NONE && (!state0 || !step))
        return fail(EBFI_ERR_ARG, "optim_step: SGD with momentum needs the momentum buffer and the step word");
    if (mom != MOM_NONE && !aligned16(state0)) return fail(EBFI_ERR_ARG, "optim_step: buffers must be 16-byte aligned");
    if (n == 0) return EBFI_OK;
    const int wd = weight_decay == 0.0 ? WD_NONE : WD_L2;
    const double maps = mom == MOM_NONE ? 3.0 : 5.0;
    float *word = mom == MOM_NONE ? nullptr : step;      // (plain SGD keeps no count: its kernel never reads one)
#define EBFI_SGD_CASE(W, M, L) \
    if (wd == W && mom == M) launch_sgd_opt<W, M>(L, maps, param, grad, state0, word, n, a, guard, flag, st)
    EBFI_SGD_CASE(WD_NONE, MOM_NONE, "optim_sgd");
    EBFI_SGD_CASE(WD_L2, MOM_NONE, "optim_sgd_l2");
    EBFI_SGD_CASE(WD_NONE, MOM_PLAIN, "optim_sgd_mom");
    EBFI_SGD_CASE(WD_L2, MOM_PLAIN, "optim_sgd_l2_mom");
    EBFI_SGD_CASE(WD_NONE, MOM_NESTEROV, "optim_sgd_nesterov");
    EBFI_SGD_CASE(WD_L2, MOM_NESTEROV, "optim_sgd_l2_nesterov");
#undef EBFI_SGD_CASE
    return check_launch("optim_sgd");
}

namespace {

template <int WD, bool AMS, bool EMA>
void launch_adam_ex(const char *label, double maps, float *p, const float *g, float *m, float *v, float *vmax, float *step,
                    int64_t n, const OptimArgs &a, int *guard, const float *flag, const float *grad_scale, float *ema,
                    float *ema_step, const EmaArgs &ea, hipStream_t st) {
    const int64_t n4 = n / 4;
    ProfScope ps(label, st, 0.0, maps * 4.0 * (double)n);
    hipLaunchKernelGGL((adam_ex_kernel<WD, AMS, EMA>), dim3((unsigned)ceil_div(std::max<int64_t>(n4, 1), 256)), dim3(256), 0, st, p,
                       g, m, v, vmax, step, n4, n, a, guard, flag, grad_scale, ema, ema_step, ea);
}

template <int WD, int MOM, bool EMA>
void launch_sgd_ex(const char *label, double maps, float *p, const float *g, float *buf, float *step, int64_t n,
                   const OptimArgs &a, int *guard, const float *flag, const float *grad_scale, float *ema, float *ema_step,
                   const EmaArgs &ea, hipStream_t st) {
    const int64_t n4 = n / 4;
    ProfScope ps(label, st, 0.0, maps * 4.0 * (double)n);
    hipLaunchKernelGGL((sgd_ex_kernel<WD, MOM, EMA>), dim3((unsigned)ceil_div(std::max<int64_t>(n4, 1), 256)), dim3(256), 0, st, p,
                       g, buf, step, n4, n, a, guard, flag, grad_scale, ema, ema_step, ea);
}

}  // namespace

extern "C" int ebfi_optim_step_ex(int kind, int flags, float *param, const float *grad, float *state0, float *state1, float *state2,
                                  float *step, int64_t n, double lr, double beta1, double beta2, double eps, double weight_decay,
                                  double momentum, double dampening, int *guard, const float *flag, const float *grad_scale,
                                  float *ema, float *ema_step, double ema_decay, int ema_warmup, void *stream) {
    if (!grad_scale && !ema)                                            // nothing to add: the launch it has always been
        return ebfi_optim_step(kind, flags, param, grad, state0, state1, state2, step, n, lr, beta1, beta2, eps, weight_decay,
                               momentum, dampening, guard, flag, stream);
    if (kind != EBFI_OPTIM_ADAM && kind != EBFI_OPTIM_SGD)
        return fail(EBFI_ERR_UNSUPPORTED, "optim_step_ex: unknown optimiser kind %d", kind);
    const int known = kind == EBFI_OPTIM_ADAM ? (EBFI_OPTIM_DECOUPLED_DECAY | EBFI_OPTIM_AMSGRAD) : EBFI_OPTIM_NESTEROV;
    if (flags & ~known) return fail(EBFI_ERR_ARG, "optim_step_ex: option flags 0x%x do not belong to optimiser kind %d", flags, kind);
    if (!(weight_decay >= 0.0)) return fail(EBFI_ERR_ARG, "optim_step_ex: weight_decay must not be negative");
    if (flag && !guard) return fail(EBFI_ERR_ARG, "optim_step_ex: an overflow flag needs the guard words");
    if (!param || !grad || n < 0) return fail(EBFI_ERR_ARG, "optim_step_ex: null argument");
    if (!aligned16(param) || !aligned16(grad)) return fail(EBFI_ERR_ARG, "optim_step_ex: buffers must be 16-byte aligned");
    if (ema) {
        if (!ema_step) return fail(EBFI_ERR_ARG, "optim_step_ex: the moving average needs its step word");
        if (!aligned16(ema)) return fail(EBFI_ERR_ARG, "optim_step_ex: buffers must be 16-byte aligned");
        if (!(ema_decay >= 0.0 && ema_decay < 1.0))
            return fail(EBFI_ERR_ARG, "optim_step_ex: ema_decay must lie in [0, 1), got %g", ema_decay);
    }
    hipStream_t st = static_cast<hipStream_t>(stream);
    const OptimArgs a{lr, beta1, beta2, eps, weight_decay, momentum, dampening};
    const EmaArgs ea{ema_decay, ema_warmup != 0 ? 1 : 0};
    const bool avg = ema != nullptr;
    const double extra = avg ? 2.0 : 0.0;
    if (kind == EBFI_OPTIM_ADAM) {
        const bool ams = (flags & EBFI_OPTIM_AMSGRAD) != 0, decoupled = (flags & EBFI_OPTIM_DECOUPLED_DECAY) != 0;
        if (!state0 || !state1 || !step || (ams && !state2))
            return fail(EBFI_ERR_ARG, "optim_step_ex: Adam needs exp_avg, exp_avg_sq%s and the step word", ams ? ", max_exp_avg_sq" : "");
        if (!aligned16(state0) || !aligned16(state1) || (ams && !aligned16(state2)))
            return fail(EBFI_ERR_ARG, "optim_step_ex: buffers must be 16-byte aligned");
        if (n == 0) return EBFI_OK;
        const int wd = weight_decay == 0.0 ? WD_NONE : decoupled ? WD_DECOUPLED : WD_L2;
        const double maps = (ams ? 9.0 : 7.0) + extra;
#define EBFI_ADAM_EX_CASE(W, A, L)                                                                                               \
    if (wd == W && ams == A) {                                                                                                   \
        if (avg) launch_adam_ex<W, A, true>(L "_ema", maps, param, grad, state0, state1, state2, step, n, a, guard, flag,       \
                                            grad_scale, ema, ema_step, ea, st);                                                  \
        else launch_adam_ex<W, A, false>(L, maps, param, grad, state0, state1, state2, step, n, a, guard, flag, grad_scale,     \
                                         nullptr, nullptr, ea, st);                                                              \
    }
        EBFI_ADAM_EX_CASE(WD_NONE, false, "optim_ex_adam")
        EBFI_ADAM_EX_CASE(WD_L2, false, "optim_ex_adam_l2")
        EBFI_ADAM_EX_CASE(WD_DECOUPLED, false, "optim_ex_adamw")
        EBFI_ADAM_EX_CASE(WD_NONE, true, "optim_ex_adam_ams")
        EBFI_ADAM_EX_CASE(WD_L2, true, "optim_ex_adam_l2_ams")
        EBFI_ADAM_EX_CASE(WD_DECOUPLED, true, "optim_ex_adamw_ams")
#undef EBFI_ADAM_EX_CASE
        return check_launch("optim_ex_adam");
    }
    const bool nesterov = (flags & EBFI_OPTIM_NESTEROV) != 0;
    if (!(momentum >= 0.0)) return fail(EBFI_ERR_ARG, "optim_step_ex: momentum must not be negative");
    if (nesterov && (momentum <= 0.0 || dampening != 0.0))
        return fail(EBFI_ERR_ARG, "optim_step_ex: Nesterov momentum requires a momentum and zero dampening");
    const int mom = momentum == 0.0 ? MOM_NONE : nesterov ? MOM_NESTEROV : MOM_PLAIN;
    if (mom != MOM_NONE && (!state0 || !step))
        return fail(EBFI_ERR_ARG, "optim_step_ex: SGD with momentum needs the momentum buffer and the step word");
    if (mom != MOM_NONE && !aligned16(state0)) return fail(EBFI_ERR_ARG, "optim_step_ex: buffers must be 16-byte aligned");
    if (n == 0) return EBFI_OK;
    const int wd = weight_decay == 0.0 ? WD_NONE : WD_L2;
    const double maps = (mom == MOM_NONE ? 3.0 : 5.0) + extra;
    float *word = mom == MOM_NONE ? nullptr : step;      // (plain SGD keeps no count: its kernel never reads one)
#define EBFI_SGD_EX_CASE(W, M, L)                                                                                                \
    if (wd == W && mom == M) {                                                                                                   \
        if (avg) launch_sgd_ex<W, M, true>(L "_ema", maps, param, grad, state0, word, n, a, guard, flag, grad_scale, ema,       \
                                           ema_step, ea, st);                                                                    \
        else launch_sgd_ex<W, M, false>(L, maps, param, grad, state0, word, n, a, guard, flag, grad_scale, nullptr, nullptr, ea, \
                                        st);                                                                                     \
    }
    EBFI_SGD_EX_CASE(WD_NONE, MOM_NONE, "optim_ex_sgd")
    EBFI_SGD_EX_CASE(WD_L2, MOM_NONE, "optim_ex_sgd_l2")
    EBFI_SGD_EX_CASE(WD_NONE, MOM_PLAIN, "optim_ex_sgd_mom")
    EBFI_SGD_EX_CASE(WD_L2, MOM_PLAIN, "optim_ex_sgd_l2_mom")
    EBFI_SGD_EX_CASE(WD_NONE, MOM_NESTEROV, "optim_ex_sgd_nesterov")
    EBFI_SGD_EX_CASE(WD_L2, MOM_NESTEROV, "optim_ex_sgd_l2_nesterov")
#undef EBFI_SGD_EX_CASE
    return check_launch("optim_ex_sgd");
}
