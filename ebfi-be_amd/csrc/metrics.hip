// Image-quality metrics of the evaluation loop (reference infer_ours.py:120-128 through loss/restore.py:43-92 and nn.MSELoss):
// per frame n of an [N, C, H, W] fp32 pair, PSNR (the reference's per-channel data range), SSIM (scikit-image
// structural_similarity with its defaults: 7x7 uniform window, sample covariance, mean over the interior cropped by 3) and MSE.
//
// Two launches, no host synchronisation, no allocation (capturable into a graph):
//   tile kernel     one wave per (plane n*C+c, strip of 128 columns, strip of TH output rows).  Lane l owns columns
//                   s + 2l, s + 2l + 1 and the wave walks the strip's TH + 6 input rows: each row is read from HBM once (one
//                   16-byte load per lane -- half the lanes pred, half target -- when the row pointers and strides allow,
//                   scalar loads otherwise), staged in LDS with 4 halo columns on each side (lanes 0-3 fetch them), and each
//                   lane reads its 8 window columns back from LDS.  The five
//                   window moments (sums of x, y, x^2, y^2, xy) are a horizontal 7-sum per row kept in a ring of 7 rows in
//                   registers; the vertical 7-sum is recomputed from the ring for every output row (no running add/subtract).
//                   Per tile it writes the SSIM-map sum over its interior pixels, the squared-error sums (plain, and of the
//                   [0, 1]-clipped pair for the one-channel PSNR), the target's max / min and a non-finite flag.
//   finalize kernel one wave per frame sums its planes' tile partials in a fixed order in fp64 and writes psnr / ssim / mse.
// No float atomics: the same inputs give bit-identical outputs.
#include "common.hpp"

#include <cmath>

using namespace ebfi;

namespace {

constexpr int MT_LANES = 64;
constexpr int MT_COLS = 2 * MT_LANES;   // output columns of a strip: 2 per lane
constexpr int MT_LDS4 = MT_COLS / 4 + 2; // float4 slots of a staged row: 4 halo columns, the strip, 4 halo columns
constexpr int MT_TH = 48;               // target output rows of a strip
constexpr int MT_PART = 6;              // doubles per tile partial (the 6th pads the record to 48 bytes)

struct MetricArgs {
    const float *pred, *target;
    int64_t ps[3], ts[3];   // strides of N, C, rows (elements); columns are unit-stride
    int C, H, W;
    int col_strips, row_strips, th;
    float c1, c2;
    double *partial;        // [N*C][row_strips][col_strips][MT_PART]
};

// 4 consecutive columns c0 .. c0 + 3 of a row, zeros outside [0, W); one 16-byte load when VEC and the 4 are inside
template <bool VEC>
__device__ __forceinline__ float4 load4(const float *row, int c0, int W) {
    if (VEC && c0 >= 0 && c0 + 3 < W) return *reinterpret_cast<const float4 *>(row + c0);
    float v[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = (c0 + j >= 0 && c0 + j < W) ? row[c0 + j] : 0.f;
    return make_float4(v[0], v[1], v[2], v[3]);
}

// 7-sums of e[1..7] and e[2..8], sharing e[2..7]
__device__ __forceinline__ void hsum2(const float e[10], float out[2]) {
    const float mid = ((e[2] + e[3]) + (e[4] + e[5])) + (e[6] + e[7]);
    out[0] = e[1] + mid;
    out[1] = mid + e[8];
}

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

template <bool VEC>
__global__ __launch_bounds__(MT_LANES) void metrics_tile_kernel(MetricArgs a) {
    __shared__ float4 stage[2][MT_LDS4];     // [pred | target][halo, strip, halo] of the current row
    const int lane = threadIdx.x;
    const int64_t tile = blockIdx.x;
    const int cs = (int)(tile % a.col_strips);
    const int rs = (int)((tile / a.col_strips) % a.row_strips);
    const int64_t plane = tile / ((int64_t)a.col_strips * a.row_strips);
    const int n = (int)(plane / a.C), c = (int)(plane - (int64_t)n * a.C);
    const int H = a.H, W = a.W;
    const int s = cs * MT_COLS, c0 = s + 2 * lane;      // this lane's output columns c0, c0 + 1
    const int r0 = rs * a.th;
    const int r1 = min(r0 + a.th, H);                  // owned rows [r0, r1)
    const int nrow = r1 - r0 + 6;                      // input rows r0 - 3 .. r1 + 2
    // loading: lanes 0-31 read 4 columns of pred, lanes 32-63 the same of target (s + 4 (lane & 31)); lanes 0-3 also read a
    // halo quad: pred / target (lane >> 1) left / right (lane & 1) of the strip
    const int arr = lane >> 5, q = lane & 31;
    const float *src = arr ? a.target + n * a.ts[0] + c * a.ts[1] : a.pred + n * a.ps[0] + c * a.ps[1];
    const int64_t rstride = arr ? a.ts[2] : a.ps[2];
    const int harr = (lane >> 1) & 1, hside = lane & 1;
    const float *hsrc = harr ? a.target + n * a.ts[0] + c * a.ts[1] : a.pred + n * a.ps[0] + c * a.ps[1];
    const int64_t hstride = harr ? a.ts[2] : a.ps[2];
    const int hcol = hside ? s + MT_COLS : s - 4;
    const bool clip = a.C == 1;
    const float inv49 = 1.f / 49.f, cov_norm = 49.f / 48.f;

    // rows in flight and the ring of horizontal moments: slot (i % 7), so that every index below is a compile-time constant
    float4 pre[7], hpre[7];
    float m[7][5][2];
#pragma unroll
    for (int k = 0; k < 7; ++k)
#pragma unroll
        for (int v = 0; v < 5; ++v) m[k][v][0] = m[k][v][1] = 0.f;

    auto fetch = [&](int i, float4 &x, float4 &h) {
        const int r = r0 - 3 + i;
        x = h = make_float4(0.f, 0.f, 0.f, 0.f);
        if (i < nrow && r >= 0 && r < H) {
            x = load4<VEC>(src + r * rstride, s + 4 * q, W);
            if (lane < 4) h = load4<VEC>(hsrc + r * hstride, hcol, W);
        }
    };

    double acc_ssim = 0.0, acc_sse = 0.0, acc_clip = 0.0;
    float tmax = -INFINITY, tmin = INFINITY;
    int bad = 0;
    constexpr int D = 2;    // prefetch distance (rows)
    fetch(0, pre[0], hpre[0]);
    fetch(1, pre[1], hpre[1]);
    for (int g = 0; g * 7 < nrow; ++g) {
#pragma unroll
        for (int k = 0; k < 7; ++k) {
            const int i = g * 7 + k;
            if (i < nrow) {                                 // (wave-uniform)
                fetch(i + D, pre[(k + D) % 7], hpre[(k + D) % 7]);
                const int r = r0 - 3 + i;
                // The workgroup is one wave, whose LDS accesses execute in program order: a compiler-only barrier keeps the
                // previous row's reads before these writes and the writes before the reads below.  (__syncthreads() would
                // also wait for the prefetched global loads of the next rows -- vmcnt(0) -- and serialise the row pipeline.)
                __builtin_amdgcn_wave_barrier();
                stage[arr][1 + q] = pre[k];
                if (lane < 4) stage[harr][hside ? MT_LDS4 - 1 : 0] = hpre[k];
                __builtin_amdgcn_wave_barrier();
                // columns c0 - 4 .. c0 + 5 of both images: floats 2 lane .. 2 lane + 9 of the staged row
                float ex[10], ey[10];
                const float2 *sx2 = reinterpret_cast<const float2 *>(stage[0]), *sy2 = reinterpret_cast<const float2 *>(stage[1]);
#pragma unroll
                for (int j = 0; j < 5; ++j) {
                    const float2 vx = sx2[lane + j], vy = sy2[lane + j];
                    ex[2 * j] = vx.x, ex[2 * j + 1] = vx.y;
                    ey[2 * j] = vy.x, ey[2 * j + 1] = vy.y;
                }
                // the lane's own pixels (ex / ey [4], [5]): squared errors, target range, non-finite values
                if (r >= r0 && r < r1) {
                    float sse = 0.f, ssc = 0.f;
#pragma unroll
                    for (int j = 0; j < 2; ++j) {
                        if (c0 + j < W) {
                            const float x = ex[4 + j], y = ey[4 + j];
                            const float d = y - x;
                            sse += d * d;
                            if (clip) {
                                const float dc = fminf(fmaxf(y, 0.f), 1.f) - fminf(fmaxf(x, 0.f), 1.f);
                                ssc += dc * dc;
                            }
                            bad |= !(isfinite(x) && isfinite(y));
                            tmax = fmaxf(tmax, y);
                            tmin = fminf(tmin, y);
                        }
                    }
                    acc_sse += (double)sse;
                    acc_clip += (double)ssc;
                }
                // horizontal 7-sums of the five moments (window columns c0 - 3 .. c0 + 4 = e[1..8])
                float exx[10], eyy[10], exy[10];
#pragma unroll
                for (int j = 1; j <= 8; ++j) {
                    exx[j] = ex[j] * ex[j];
                    eyy[j] = ey[j] * ey[j];
                    exy[j] = ex[j] * ey[j];
                }
                hsum2(ex, m[k][0]);
                hsum2(ey, m[k][1]);
                hsum2(exx, m[k][2]);
                hsum2(eyy, m[k][3]);
                hsum2(exy, m[k][4]);
                // vertical 7-sum for output row r - 3, recomputed from the ring in slot order
                const int ro = r - 3;
                if (i >= 6 && ro >= 3 && ro < H - 3) {
                    float ssum = 0.f;
#pragma unroll
                    for (int j = 0; j < 2; ++j) {
                        float v[5];
#pragma unroll
                        for (int t = 0; t < 5; ++t)
                            v[t] = ((m[0][t][j] + m[1][t][j]) + (m[2][t][j] + m[3][t][j])) + ((m[4][t][j] + m[5][t][j]) + m[6][t][j]);
                        const float ux = v[0] * inv49, uy = v[1] * inv49;
                        const float vx = cov_norm * (v[2] * inv49 - ux * ux);
                        const float vy = cov_norm * (v[3] * inv49 - uy * uy);
                        const float vxy = cov_norm * (v[4] * inv49 - ux * uy);
                        const float num = (2.f * ux * uy + a.c1) * (2.f * vxy + a.c2);
                        const float den = (ux * ux + uy * uy + a.c1) * (vx + vy + a.c2);
                        if (c0 + j >= 3 && c0 + j < W - 3) ssum += num / den;
                    }
                    acc_ssim += (double)ssum;
                }
            }
        }
    }
    acc_ssim = wave_sum(acc_ssim);
    acc_sse = wave_sum(acc_sse);
    acc_clip = wave_sum(acc_clip);
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        tmax = fmaxf(tmax, __shfl_xor(tmax, d, 64));
        tmin = fminf(tmin, __shfl_xor(tmin, d, 64));
        bad |= __shfl_xor(bad, d, 64);
    }
    if (lane == 0) {
        double *p = a.partial + tile * MT_PART;
        const double qnan = __builtin_nan("");
        p[0] = bad ? qnan : acc_ssim;
        p[1] = bad ? qnan : acc_sse;
        p[2] = bad ? qnan : acc_clip;
        p[3] = (double)tmax;
        p[4] = (double)tmin;
        p[5] = 0.0;
    }
}

// one wave per frame: fixed-order fp64 sums of the tile partials of its C planes
struct PlaneSums {
    double ssim, sse, sse_clip, tmax, tmin;
};

__device__ PlaneSums plane_sums(const double *__restrict__ p, int64_t tiles) {
    PlaneSums s{0.0, 0.0, 0.0, -INFINITY, INFINITY};
    for (int64_t t = threadIdx.x; t < tiles; t += MT_LANES) {
        const double *q = p + t * MT_PART;
        s.ssim += q[0];
        s.sse += q[1];
        s.sse_clip += q[2];
        s.tmax = fmax(s.tmax, q[3]);
        s.tmin = fmin(s.tmin, q[4]);
    }
    s.ssim = wave_sum(s.ssim);
    s.sse = wave_sum(s.sse);
    s.sse_clip = wave_sum(s.sse_clip);
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        s.tmax = fmax(s.tmax, __shfl_xor(s.tmax, d, 64));
        s.tmin = fmin(s.tmin, __shfl_xor(s.tmin, d, 64));
    }
    return s;
}

__global__ __launch_bounds__(MT_LANES) void metrics_finalize_kernel(const double *__restrict__ partial, int C, int H, int W,
                                                                    int64_t tiles_per_plane, float *__restrict__ psnr,
                                                                    float *__restrict__ ssim, float *__restrict__ mse) {
    const int n = blockIdx.x;
    const double hw = (double)H * (double)W, interior = (double)(H - 6) * (double)(W - 6);
    const double *base = partial + (int64_t)n * C * tiles_per_plane * MT_PART;
    // PSNR's data range of channel c is max(target_c) - min(target over ALL channels) (loss/restore.py:84): the first pass
    // takes the all-channel min, the second evaluates the channels (the partials are re-read, not kept in a private array)
    double tmin_all = INFINITY;
    for (int c = 0; c < C; ++c) tmin_all = fmin(tmin_all, plane_sums(base + c * tiles_per_plane * MT_PART, tiles_per_plane).tmin);
    double ssim_sum = 0.0, sse_all = 0.0, psnr_sum = 0.0;
    for (int c = 0; c < C; ++c) {
        const PlaneSums s = plane_sums(base + c * tiles_per_plane * MT_PART, tiles_per_plane);
        ssim_sum += s.ssim / interior;
        sse_all += s.sse;
        // C == 1: the reference's 2-D branch, both images clipped to [0, 1] and data range 1
        const double dr = C == 1 ? 1.0 : s.tmax - tmin_all;
        psnr_sum += 10.0 * log10((dr * dr) / ((C == 1 ? s.sse_clip : s.sse) / hw));
    }
    if (threadIdx.x == 0) {
        // a non-finite value anywhere in a plane made its tile write NaN sums: every metric of the frame is NaN
        const bool bad = isnan(ssim_sum) || isnan(sse_all);
        const float qnan = __builtin_nanf("");
        psnr[n] = bad ? qnan : (float)(psnr_sum / C);
        ssim[n] = bad ? qnan : (float)(ssim_sum / C);
        mse[n] = bad ? qnan : (float)(sse_all / ((double)C * hw));
    }
}

struct MetricGrid {
    int col_strips, row_strips, th;
    int64_t tiles_per_plane;
};

MetricGrid metric_grid(int H, int W) {
    MetricGrid g;
    g.col_strips = (int)ceil_div(W, MT_COLS);
    g.row_strips = (int)ceil_div(H, MT_TH);
    g.th = (int)ceil_div(H, g.row_strips);
    g.tiles_per_plane = (int64_t)g.col_strips * g.row_strips;
    return g;
}

}  // namespace

extern "C" int64_t ebfi_image_metrics_workspace(int64_t N, int C, int H, int W) {
    if (N < 0 || C < 1 || H < 1 || W < 1) return 0;
    return N * C * metric_grid(H, W).tiles_per_plane * MT_PART * (int64_t)sizeof(double);
}

extern "C" int ebfi_image_metrics(const float *pred, const int64_t pred_strides[4], const float *target,
                                  const int64_t target_strides[4], int64_t N, int C, int H, int W, float ssim_data_range,
                                  void *workspace, int64_t workspace_bytes, float *out_psnr, float *out_ssim, float *out_mse,
                                  void *stream) {
    if (!pred || !target || !pred_strides || !target_strides || !workspace || !out_psnr || !out_ssim || !out_mse)
        return fail(EBFI_ERR_ARG, "image_metrics: null argument");
    if (N < 0 || C < 1 || H < 7 || W < 7)
        return fail(EBFI_ERR_ARG, "image_metrics: bad shape N=%lld C=%d H=%d W=%d (C >= 1; H, W >= 7: the SSIM window is 7x7)",
                    (long long)N, C, H, W);
    if (!(ssim_data_range > 0.f) || !std::isfinite(ssim_data_range))
        return fail(EBFI_ERR_ARG, "image_metrics: ssim_data_range must be positive and finite");
    if (pred_strides[3] != 1 || target_strides[3] != 1)
        return fail(EBFI_ERR_UNSUPPORTED, "image_metrics: the column stride must be 1 (got %lld / %lld)", (long long)pred_strides[3],
                    (long long)target_strides[3]);
    const int64_t need = ebfi_image_metrics_workspace(N, C, H, W);
    if (workspace_bytes < need)
        return fail(EBFI_ERR_WORKSPACE, "image_metrics: workspace %lld bytes, %lld needed", (long long)workspace_bytes, (long long)need);
    if (!aligned16(workspace)) return fail(EBFI_ERR_ARG, "image_metrics: workspace must be 16-byte aligned");
    if (N == 0) return EBFI_OK;
    const MetricGrid g = metric_grid(H, W);
    const int64_t tiles = N * C * g.tiles_per_plane;
    if (tiles > INT32_MAX || N > INT32_MAX) return fail(EBFI_ERR_ARG, "image_metrics: too many tiles (%lld)", (long long)tiles);
    MetricArgs a;
    a.pred = pred;
    a.target = target;
    bool vec = aligned16(pred) && aligned16(target);
    for (int d = 0; d < 3; ++d) {
        a.ps[d] = pred_strides[d];
        a.ts[d] = target_strides[d];
        vec = vec && (pred_strides[d] % 4 == 0) && (target_strides[d] % 4 == 0);
    }
    a.C = C, a.H = H, a.W = W;
    a.col_strips = g.col_strips, a.row_strips = g.row_strips, a.th = g.th;
    a.c1 = (0.01f * ssim_data_range) * (0.01f * ssim_data_range);
    a.c2 = (0.03f * ssim_data_range) * (0.03f * ssim_data_range);
    a.partial = static_cast<double *>(workspace);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const double bytes = 8.0 * (double)N * C * H * (double)W;
    {
        ProfScope ps(vec ? "metrics_tile/vec" : "metrics_tile/narrow", st, 0.0, bytes);
        if (vec)
            hipLaunchKernelGGL(metrics_tile_kernel<true>, dim3((unsigned)tiles), dim3(MT_LANES), 0, st, a);
        else
            hipLaunchKernelGGL(metrics_tile_kernel<false>, dim3((unsigned)tiles), dim3(MT_LANES), 0, st, a);
    }
    int rc = check_launch("metrics_tile");
    if (rc != EBFI_OK) return rc;
    {
        ProfScope ps("metrics_finalize", st, 0.0, (double)tiles * MT_PART * 8.0);
        hipLaunchKernelGGL(metrics_finalize_kernel, dim3((unsigned)N), dim3(MT_LANES), 0, st, (const double *)workspace, C, H, W,
                           g.tiles_per_plane, out_psnr, out_ssim, out_mse);
    }
    return check_launch("metrics_finalize");
}
