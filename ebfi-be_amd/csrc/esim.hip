// The event simulator of the synthetic-dataset step: what generate_dataset/syn_gopro.py:77-81,115-116 asks of
// esim_py.EventSimulator, on the device.  esim_py is not part of the reference tree; the law is written out in
// include/ebfi_hip.h and restated in float64 numpy by tests/esim_ref.py, and these kernels give that restatement's bits.
//
// One lane owns one pixel and walks the frames of a chunk with `it`, `ref` and `last_t` in registers; lanes run along x (over
// the flattened [y][x] index), so a wave reads 64 consecutive bytes of a row per frame and writes 64 consecutive counts.  The
// chunk is walked twice:
//   count  writes counts[k][y][x], the events of the pixel in interval k, and leaves the state alone;
//   emit   gets the exclusive prefix sums of those counts, walks again and stores every event at its own index, then writes
//          the state.  Exact allocation, no atomics, no overflow path, the same layout every run.  The caller then sorts
//          stably by pixel and by t: the law's order (t, y, x, emission), also where events of two intervals tie in t.
// Both passes are the SAME template (esim_walk<EMIT, BGR>), so the two walks cannot disagree.
//
// Rounding.  t = T_prev + ((cross - it) * dt) / (itdt - it) rounds after the multiply, after the divide and after the add, as
// the float64 restatement does.  hipcc contracts a * b + c into one fused operation by default, which would change the last
// bits of `t` (and of `cross = cross + pol * C` if it were written as a product): contraction is switched off for this file,
// and the division is hipcc's correctly rounded default (the library is built without fast-math).  The kernels never call
// log: the level of a byte comes from the caller's 256-entry float64 table, the same bits the restatement reads.
//
// Termination.  The crossing loop is a counted `for` to the bound the host computes from the table and the thresholds
// (ebfi_esim_loop_bound); thresholds below 1e-3, non-finite values and times that do not increase never reach the GPU.
//
// from_bgr: gray = (4899 R + 9617 G + 1868 B + 8192) >> 14, OpenCV's 8-bit BGR -> GRAY fixed point (what cv2.imread of a
// colour file in grayscale mode, hence esim_py's folder reader, would give).  cv2 is not installed where this is tested, so
// the constant set is pinned by the restatement only.
#include <cmath>

#include "common.hpp"

#pragma clang fp contract(off)

using namespace ebfi;

namespace {

constexpr int kThreads = 256;
constexpr int64_t kMaxBound = (int64_t)1 << 24;

struct Table {   // kernel arguments: the level of every byte, and the chunk's frame times (T[0] = where the state stands)
    double L[256];
    double T[EBFI_ESIM_MAX_CHUNK + 1];
};

struct Thresholds {
    double Cp, Cn, refractory;
    int bound;
};

template <bool BGR>
__device__ inline int gray_at(const uint8_t *p) {
    if constexpr (BGR) {
        const int b = p[0], g = p[1], r = p[2];
        return (4899 * r + 9617 * g + 1868 * b + 8192) >> 14;
    } else {
        return p[0];
    }
}

// the table is indexed per lane: 2 KiB of LDS per workgroup, filled from the kernel arguments
__device__ inline void stage_levels(const Table &tab, double *lds) {
    for (int i = threadIdx.x; i < 256; i += kThreads) lds[i] = tab.L[i];
    __syncthreads();
}

// grid: ceil(H * W / kThreads) workgroups; thread p owns pixel (p / W, p % W).
// state: it / ref / last_t planes of H * W doubles each (emit reads and writes the same planes: no __restrict__).
// EMIT: offsets [n][H * W], events stored below `capacity` only.
template <bool EMIT, bool BGR>
__global__ __launch_bounds__(kThreads) void esim_walk(const uint8_t *__restrict__ frames, int64_t sf, int64_t sr, int n, int H,
                                                      int W, Table tab, Thresholds th, const double *state_in,
                                                      double *state_out, int32_t *__restrict__ counts,
                                                      const int64_t *__restrict__ offsets, int64_t capacity,
                                                      int16_t *__restrict__ xs, int16_t *__restrict__ ys,
                                                      double *__restrict__ ts, int8_t *__restrict__ ps) {
    __shared__ double level[256];
    stage_levels(tab, level);
    const int64_t HW = (int64_t)H * W;
    const int64_t p = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (p >= HW) return;
    const int y = (int)(p / W), x = (int)(p % W);
    const uint8_t *src = frames + (int64_t)y * sr + (int64_t)x * (BGR ? 3 : 1);

    double it = state_in[p], ref = state_in[HW + p], last_t = state_in[2 * HW + p];
    int v_next = gray_at<BGR>(src);
    for (int k = 0; k < n; ++k) {
        const int v = v_next;
        if (k + 1 < n) v_next = gray_at<BGR>(src + (int64_t)(k + 1) * sf);   // (the next frame's byte is in flight during the walk)
        const double t_prev = tab.T[k];
        const double dt = tab.T[k + 1] - t_prev;
        const double itdt = level[v];
        int emitted = 0;
        int64_t at = 0;
        if constexpr (EMIT) at = offsets[(int64_t)k * HW + p];
        if (fabs(it - itdt) > 1e-6) {
            const bool up = itdt >= it;
            const double step = up ? th.Cp : -th.Cn;   // pol * C: pol is +-1, the product is exact
            const double den = itdt - it;
            double cross = ref;
            for (int i = 0; i < th.bound; ++i) {
                cross = cross + step;
                const bool inside = up ? (cross > it && cross <= itdt) : (cross < it && cross >= itdt);
                if (!inside) break;
                const double num = (cross - it) * dt;
                const double q = num / den;
                const double t = t_prev + q;
                if (last_t == 0.0 || (t - last_t) >= th.refractory) {
                    if constexpr (EMIT) {
                        const int64_t e = at + emitted;
                        if ((uint64_t)e < (uint64_t)capacity) {   // (one compare: a negative index is refused too)
                            xs[e] = (int16_t)x;
                            ys[e] = (int16_t)y;
                            ts[e] = t;
                            ps[e] = (int8_t)(up ? 1 : -1);
                        }
                    }
                    ++emitted;
                    last_t = t;
                }
                ref = cross;
            }
        }
        it = itdt;
        if constexpr (!EMIT) counts[(int64_t)k * HW + p] = emitted;
    }
    if constexpr (EMIT) {
        state_out[p] = it;
        state_out[HW + p] = ref;
        state_out[2 * HW + p] = last_t;
    }
}

template <bool BGR>
__global__ __launch_bounds__(kThreads) void esim_init(const uint8_t *__restrict__ frame, int64_t sr, int H, int W, Table tab,
                                                      double *__restrict__ state) {
    __shared__ double level[256];
    stage_levels(tab, level);
    const int64_t HW = (int64_t)H * W;
    const int64_t p = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (p >= HW) return;
    const int y = (int)(p / W), x = (int)(p % W);
    const double l = level[gray_at<BGR>(frame + (int64_t)y * sr + (int64_t)x * (BGR ? 3 : 1))];
    state[p] = l;
    state[HW + p] = l;
    state[2 * HW + p] = 0.0;
}

bool levels_ok(const double *levels, double *lo, double *hi) {
    *lo = *hi = levels[0];
    for (int v = 0; v < 256; ++v) {
        if (!std::isfinite(levels[v])) return false;
        if (levels[v] < *lo) *lo = levels[v];
        if (levels[v] > *hi) *hi = levels[v];
    }
    return true;
}

int check_frame_args(const char *what, const void *frames, const double *levels, const void *state, int H, int W) {
    if (!frames || !levels || !state) return fail(EBFI_ERR_ARG, "%s: null pointer", what);
    if (H < 1 || H > 32767 || W < 1 || W > 32767)
        return fail(EBFI_ERR_ARG, "%s: H = %d, W = %d outside [1, 32767] (coordinates are int16)", what, H, W);
    return EBFI_OK;
}

// everything ebfi_esim_count and ebfi_esim_emit have in common; fills the kernel arguments
int check_walk_args(const char *what, const uint8_t *frames, const int64_t *strides, int64_t n, int H, int W, const double *times,
                    const double *levels, double Cp, double Cn, double refractory, const double *state, Table *tab,
                    Thresholds *th) {
    const int rc = check_frame_args(what, frames, levels, state, H, W);
    if (rc != EBFI_OK) return rc;
    if (!strides || !times) return fail(EBFI_ERR_ARG, "%s: null pointer", what);
    if (n < 0 || n > EBFI_ESIM_MAX_CHUNK)
        return fail(EBFI_ERR_ARG, "%s: n = %lld outside [0, %d] (feed a longer sequence in chunks)", what, (long long)n,
                    EBFI_ESIM_MAX_CHUNK);
    if (strides[0] < 0 || strides[1] < 0) return fail(EBFI_ERR_ARG, "%s: strides must be >= 0", what);
    if (!std::isfinite(refractory) || refractory < 0.0)
        return fail(EBFI_ERR_ARG, "%s: refractory_period must be finite and >= 0", what);
    const int64_t bound = ebfi_esim_loop_bound(levels, Cp, Cn);
    if (bound < 0)
        return fail(EBFI_ERR_ARG, "%s: Cp = %g, Cn = %g must be finite and >= 1e-3, the levels finite (log_eps > 0), and "
                                  "(max L - min L) / min(Cp, Cn) at most 2^24", what, Cp, Cn);
    for (int64_t k = 0; k <= n; ++k) {
        if (!std::isfinite(times[k])) return fail(EBFI_ERR_ARG, "%s: times[%lld] is not finite", what, (long long)k);
        if (k > 0 && !(times[k] > times[k - 1]))
            return fail(EBFI_ERR_ARG, "%s: times must increase strictly (times[%lld] = %.17g after %.17g)", what, (long long)k,
                        times[k], times[k - 1]);
        tab->T[k] = times[k];
    }
    for (int64_t k = n + 1; k <= EBFI_ESIM_MAX_CHUNK; ++k) tab->T[k] = 0.0;
    for (int v = 0; v < 256; ++v) tab->L[v] = levels[v];
    th->Cp = Cp, th->Cn = Cn, th->refractory = refractory, th->bound = (int)bound;
    return EBFI_OK;
}

}  // namespace

extern "C" int64_t ebfi_esim_loop_bound(const double *levels, double Cp, double Cn) {
    double lo, hi;
    if (!levels || !levels_ok(levels, &lo, &hi)) return -1;
    if (!std::isfinite(Cp) || !std::isfinite(Cn) || Cp < 1e-3 || Cn < 1e-3) return -1;
    const double rounds = std::ceil((hi - lo) / (Cp < Cn ? Cp : Cn));
    if (!(rounds <= (double)kMaxBound)) return -1;
    return (int64_t)rounds + 1;
}

extern "C" int ebfi_esim_init(const uint8_t *frame, int64_t row_stride, int from_bgr, int H, int W, const double *levels,
                              double *state, void *stream) {
    const int rc = check_frame_args("esim_init", frame, levels, state, H, W);
    if (rc != EBFI_OK) return rc;
    if (row_stride < 0) return fail(EBFI_ERR_ARG, "esim_init: strides must be >= 0");
    double lo, hi;
    if (!levels_ok(levels, &lo, &hi)) return fail(EBFI_ERR_ARG, "esim_init: the levels must be finite (log_eps > 0)");
    Table tab = {};
    for (int v = 0; v < 256; ++v) tab.L[v] = levels[v];
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int64_t HW = (int64_t)H * W;
    const dim3 grid((unsigned)ceil_div(HW, kThreads)), block(kThreads);
    {
        ProfScope ps_("esim_init", st, 0.0, (double)HW * ((from_bgr ? 3.0 : 1.0) + 24.0));
        if (from_bgr)
            hipLaunchKernelGGL(esim_init<true>, grid, block, 0, st, frame, row_stride, H, W, tab, state);
        else
            hipLaunchKernelGGL(esim_init<false>, grid, block, 0, st, frame, row_stride, H, W, tab, state);
    }
    return check_launch("esim_init");
}

extern "C" int ebfi_esim_count(const uint8_t *frames, const int64_t frame_strides[2], int from_bgr, int64_t n, int H, int W,
                               const double *times, const double *levels, double Cp, double Cn, double refractory_period,
                               const double *state, int32_t *counts, void *stream) {
    Table tab;
    Thresholds th;
    const int rc = check_walk_args("esim_count", frames, frame_strides, n, H, W, times, levels, Cp, Cn, refractory_period, state,
                                   &tab, &th);
    if (rc != EBFI_OK) return rc;
    if (!counts) return fail(EBFI_ERR_ARG, "esim_count: null pointer");
    if (n == 0) return EBFI_OK;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int64_t HW = (int64_t)H * W;
    const dim3 grid((unsigned)ceil_div(HW, kThreads)), block(kThreads);
    {
        ProfScope ps_("esim_walk/count", st, 0.0, (double)HW * ((double)n * ((from_bgr ? 3.0 : 1.0) + 4.0) + 24.0));
        if (from_bgr)
            hipLaunchKernelGGL((esim_walk<false, true>), grid, block, 0, st, frames, frame_strides[0], frame_strides[1], (int)n, H,
                               W, tab, th, state, nullptr, counts, nullptr, (int64_t)0, nullptr, nullptr, nullptr, nullptr);
        else
            hipLaunchKernelGGL((esim_walk<false, false>), grid, block, 0, st, frames, frame_strides[0], frame_strides[1], (int)n,
                               H, W, tab, th, state, nullptr, counts, nullptr, (int64_t)0, nullptr, nullptr, nullptr, nullptr);
    }
    return check_launch("esim_count");
}

extern "C" int ebfi_esim_emit(const uint8_t *frames, const int64_t frame_strides[2], int from_bgr, int64_t n, int H, int W,
                              const double *times, const double *levels, double Cp, double Cn, double refractory_period,
                              double *state, const int64_t *offsets, int64_t capacity, int16_t *xs, int16_t *ys, double *ts,
                              int8_t *ps, void *stream) {
    Table tab;
    Thresholds th;
    const int rc = check_walk_args("esim_emit", frames, frame_strides, n, H, W, times, levels, Cp, Cn, refractory_period, state,
                                   &tab, &th);
    if (rc != EBFI_OK) return rc;
    if (capacity < 0) return fail(EBFI_ERR_ARG, "esim_emit: capacity %lld < 0", (long long)capacity);
    if (!offsets || (capacity > 0 && (!xs || !ys || !ts || !ps))) return fail(EBFI_ERR_ARG, "esim_emit: null pointer");
    if (n == 0) return EBFI_OK;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int64_t HW = (int64_t)H * W;
    const dim3 grid((unsigned)ceil_div(HW, kThreads)), block(kThreads);
    {
        ProfScope ps_("esim_walk/emit", st, 0.0,
                      (double)HW * ((double)n * ((from_bgr ? 3.0 : 1.0) + 8.0) + 48.0) + (double)capacity * 13.0);
        if (from_bgr)
            hipLaunchKernelGGL((esim_walk<true, true>), grid, block, 0, st, frames, frame_strides[0], frame_strides[1], (int)n, H,
                               W, tab, th, state, state, nullptr, offsets, capacity, xs, ys, ts, ps);
        else
            hipLaunchKernelGGL((esim_walk<true, false>), grid, block, 0, st, frames, frame_strides[0], frame_strides[1], (int)n, H,
                               W, tab, th, state, state, nullptr, offsets, capacity, xs, ys, ts, ps);
    }
    return check_launch("esim_emit");
}
