// Deformable position-sensitive ROI pooling: the second op of the reference's DCNv2 package
// (models/DCNv2/src/cuda/dcn_v2_psroi_pooling_cuda.cu).  The law is written out in include/ebfi_hip.h and restated in numpy
// by tests/psroi_ref.py; these kernels give that restatement's sample positions bit for bit.
//
// Geometry once per (ROI, class).  Where a sample lands depends on (n, cls, ph, pw, ih, iw) and not on the channel; the
// reference recomputes it for every output element, D / nc times too often.  A workgroup owns one (ROI, class) -- in the
// forward a chunk of its channels -- and first fills an LDS table with one entry per sample: the validity flag, the plane
// offsets of the corners (floor, floor) and (ceil, ceil), dx and dy.  The other two corners follow from them: ceil(w) and
// floor(w) differ exactly when dx > 0.  Per bin the table also keeps the group cell gh * G + gw, the part cell and the
// count.  P * P * spp * spp entries (784 at P = 7, spp = 4) fit one tile of kTile; a larger pooling walks its bins in tiles.
// A skipped sample, a bin that nothing reached and an ROI whose batch index is out of range keep offsets 0 and a cleared flag:
// every load is in bounds and the value is dropped by a select, never by a branch around the address.
//
// forward   spp == 4: a bin's 16 samples are the 16 lanes of one DPP row; the 16 rows of a workgroup walk the flattened
//           (channel, bin) items of the tile and each sums its bin with row shifts, in the law's sample order.  Any other
//           spp: one lane per item, the samples in a loop.
// backward  one workgroup per (ROI, class), in four channel groups; a lane keeps its table entries and walks every fourth
//           channel of the class.  grad_input is scattered with float atomics into the tensor the host zeroed.  The trans
//           gradient of an entry is summed over a group's channels in a register in channel order, over the groups in LDS in
//           group order; the entries of a bin and then the bins of a part cell (part < P makes bins share one) are summed
//           from LDS in index order by the one lane that owns the cell: one writer, one order, the same bits every call.
//
// Rounding.  Every step of the coordinate law is one fp32 operation; hipcc would contract a * b + c into one fused operation
// and move samples across the -0.5 / W - 0.5 boundaries and the integer grid, so contraction is off for this file (the
// convention of esim.hip), and the divisions are hipcc's correctly rounded default.
#include <algorithm>
#include <climits>
#include <cmath>

#include "common.hpp"

#pragma clang fp contract(off)

using namespace ebfi;

namespace {

constexpr int kThreads = 256;
constexpr int kTile = 1024;                    // table entries of one tile
constexpr int kPerLane = kTile / kThreads;     // entries a lane of the backward keeps
constexpr int kBwdGroups = 4;                  // channel groups of a backward workgroup (kBwdGroups * kThreads lanes)
constexpr int kMaxSpp = 32;                    // spp * spp <= kTile: a bin never straddles two tiles

struct PoolArgs {
    int B, C, H, W, R, nc, no_trans, D, G, P, part, spp;
    float scale, trans_std;
};

struct Table {
    int o00[kTile], o11[kTile], ok[kTile];     // per sample: offsets of (y0, x0) and (y1, x1) in a plane, validity
    float dx[kTile], dy[kTile];
    int gcell[kTile], pcell[kTile];            // per bin: gh * G + gw and part_h * part + part_w
    float cnt[kTile];                          // per bin: samples that contribute
};

struct Roi {
    int b;
    bool ok;
    float sw, sh, rw, rh, bw, bh, sbw, sbh;
};

__device__ inline Roi roi_geometry(const float *__restrict__ rois, int n, const PoolArgs &a) {
    const float *r = rois + (int64_t)n * 5;
    Roi g;
    const float bf = r[0];
    g.ok = bf >= 0.f && bf < (float)a.B && bf == floorf(bf);   // (NaN fails every compare)
    g.b = g.ok ? (int)bf : 0;
    g.sw = roundf(r[1]) * a.scale - 0.5f;
    g.sh = roundf(r[2]) * a.scale - 0.5f;
    const float ew = (roundf(r[3]) + 1.f) * a.scale - 0.5f;
    const float eh = (roundf(r[4]) + 1.f) * a.scale - 0.5f;
    g.rw = fmaxf(ew - g.sw, 0.1f);
    g.rh = fmaxf(eh - g.sh, 0.1f);
    g.bw = g.rw / (float)a.P;
    g.bh = g.rh / (float)a.P;
    g.sbw = g.bw / (float)a.spp;
    g.sbh = g.bh / (float)a.spp;
    return g;
}

__device__ inline int clampi(int v, int lo, int hi) { return min(max(v, lo), hi); }

// part cell of a bin; the clamp is for memory safety only (float(ph) / P * part < part for every P the launch accepts)
__device__ inline int part_cell(int ph, int pw, const PoolArgs &a) {
    const int part_h = clampi((int)floorf((float)ph / (float)a.P * (float)a.part), 0, a.part - 1);
    const int part_w = clampi((int)floorf((float)pw / (float)a.P * (float)a.part), 0, a.part - 1);
    return part_h * a.part + part_w;
}

// Fills the table for bins [bin0, bin0 + nb) of (n, cls) with the whole workgroup, whatever its size; ends with a barrier.
__device__ void fill_table(Table &T, const Roi &g, const float *__restrict__ trans, int n, int cls, int bin0, int nb,
                           const PoolArgs &a) {
    const int spp2 = a.spp * a.spp, part2 = a.part * a.part;
    const float wmax = (float)a.W - 0.5f, hmax = (float)a.H - 0.5f;
    const float wlast = (float)a.W - 1.f, hlast = (float)a.H - 1.f;
    for (int bl = threadIdx.x; bl < nb; bl += blockDim.x) {
        const int ph = (bin0 + bl) / a.P, pw = (bin0 + bl) % a.P;
        const int gw = clampi((int)floorf((float)pw * (float)a.G / (float)a.P), 0, a.G - 1);
        const int gh = clampi((int)floorf((float)ph * (float)a.G / (float)a.P), 0, a.G - 1);
        T.gcell[bl] = gh * a.G + gw;
        T.pcell[bl] = part_cell(ph, pw, a);
    }
    for (int e = threadIdx.x; e < nb * spp2; e += blockDim.x) {
        const int bl = e / spp2, s = e % spp2;
        const int ih = s / a.spp, iw = s % a.spp;
        const int ph = (bin0 + bl) / a.P, pw = (bin0 + bl) % a.P;
        float tx = 0.f, ty = 0.f;
        if (!a.no_trans) {
            const float *t = trans + ((int64_t)(n * a.nc + cls) * 2) * part2 + part_cell(ph, pw, a);
            tx = t[0] * a.trans_std;
            ty = t[part2] * a.trans_std;
        }
        float w0 = (float)pw * g.bw + g.sw;
        w0 += tx * g.rw;
        float h0 = (float)ph * g.bh + g.sh;
        h0 += ty * g.rh;
        float w = w0 + (float)iw * g.sbw;
        float h = h0 + (float)ih * g.sbh;
        const bool skip = w < -0.5f || w > wmax || h < -0.5f || h > hmax;
        const bool ok = g.ok && !skip;
        w = fminf(fmaxf(w, 0.f), wlast);   // finite and inside the map from here on, whatever came in (NaN -> 0)
        h = fminf(fmaxf(h, 0.f), hlast);
        const float fw = floorf(w), fh = floorf(h);
        const int x0 = (int)fw, x1 = (int)ceilf(w), y0 = (int)fh, y1 = (int)ceilf(h);
        T.ok[e] = ok ? 1 : 0;
        T.o00[e] = ok ? y0 * a.W + x0 : 0;
        T.o11[e] = ok ? y1 * a.W + x1 : 0;
        T.dx[e] = ok ? w - fw : 0.f;
        T.dy[e] = ok ? h - fh : 0.f;
    }
    __syncthreads();
    for (int bl = threadIdx.x; bl < nb; bl += blockDim.x) {
        int c = 0;
        for (int s = 0; s < spp2; ++s) c += T.ok[bl * spp2 + s];
        T.cnt[bl] = (float)c;
    }
    __syncthreads();
}

struct Sample {
    float v00, v01, v10, v11, dx, dy;
    int o00, o01, o10, o11;
    bool ok;
};

// the four corners of table entry e in `plane`: U00 = (y0, x0), U01 = (y1, x0), U10 = (y0, x1), U11 = (y1, x1)
__device__ inline Sample gather(const Table &T, int e, const float *__restrict__ plane) {
    Sample q;
    q.dx = T.dx[e], q.dy = T.dy[e], q.ok = T.ok[e] != 0;
    const int step = q.dx > 0.f ? 1 : 0;   // ceil(w) - floor(w)
    q.o00 = T.o00[e], q.o11 = T.o11[e];
    q.o10 = q.o00 + step, q.o01 = q.o11 - step;
    q.v00 = plane[q.o00], q.v01 = plane[q.o01], q.v10 = plane[q.o10], q.v11 = plane[q.o11];
    return q;
}

__device__ inline float bilinear(const Sample &q) {
    const float v = (1.f - q.dx) * (1.f - q.dy) * q.v00 + (1.f - q.dx) * q.dy * q.v01 + q.dx * (1.f - q.dy) * q.v10 +
                    q.dx * q.dy * q.v11;
    return q.ok ? v : 0.f;
}

// One step of the row scan: v + (the running sum of the lane below in the 16-lane DPP row; 0 below lane 0).
__device__ inline float row_scan_step(float v, float acc) {
    return v + __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(acc), 0x111 /* row_shr:1 */, 0xf, 0xf, true));
}

// Lane 15 of every DPP row gets ((v0 + v1) + v2) + ... + v15: the law's summation order (ih outer, iw inner), so the
// pooled value has the bits of the fp32 restatement, not only its count.  All 64 lanes of the wave must be active.
__device__ inline float row_sum16_in_order(float v) {
    float acc = v;
#pragma unroll
    for (int k = 0; k < 15; ++k) acc = row_scan_step(v, acc);
    return acc;
}

// grid: R * nc * nchunk workgroups; workgroup (n, cls, chunk) pools channels [cls * cec + chunk * chunk_c, + chunk_c) of ROI n.
template <bool SPP4>
__global__ __launch_bounds__(kThreads) void psroi_forward(const float *__restrict__ in, const float *__restrict__ rois,
                                                          const float *__restrict__ trans, float *__restrict__ out,
                                                          float *__restrict__ count, PoolArgs a, int nchunk, int chunk_c) {
    __shared__ Table T;
    const int cec = a.D / a.nc;
    int wg = blockIdx.x;
    const int chunk = wg % nchunk;
    wg /= nchunk;
    const int cls = wg % a.nc, n = wg / a.nc;
    const int d0 = cls * cec + chunk * chunk_c;
    const int nd = min(chunk_c, cec - chunk * chunk_c);
    const Roi g = roi_geometry(rois, n, a);
    const int PP = a.P * a.P, spp2 = a.spp * a.spp, GG = a.G * a.G, bpt = kTile / spp2;
    const int64_t HW = (int64_t)a.H * a.W;
    const float *base = in + (int64_t)g.b * a.C * HW;

    for (int bin0 = 0; bin0 < PP; bin0 += bpt) {
        const int nb = min(bpt, PP - bin0);
        fill_table(T, g, trans, n, cls, bin0, nb, a);
        const int items = nd * nb;   // (channel, bin), bin fastest: consecutive items store consecutive outputs
        if constexpr (SPP4) {
            const int row = threadIdx.x >> 4, s = threadIdx.x & 15;
            for (int it0 = 0; it0 < items; it0 += kThreads / 16) {   // (uniform trip count: the row sums need every lane)
                const bool live = it0 + row < items;
                const int it = live ? it0 + row : 0;
                const int d = d0 + it / nb, bl = it % nb;
                const Sample q = gather(T, bl * 16 + s, base + ((int64_t)d * GG + T.gcell[bl]) * HW);
                const float sum = row_sum16_in_order(bilinear(q));
                if (live && s == 15) {
                    const float c = T.cnt[bl];
                    const int64_t o = ((int64_t)n * a.D + d) * PP + bin0 + bl;
                    out[o] = c > 0.f ? sum / c : 0.f;
                    if (count) count[o] = c;
                }
            }
        } else {
            for (int it = threadIdx.x; it < items; it += kThreads) {
                const int d = d0 + it / nb, bl = it % nb;
                const float *plane = base + ((int64_t)d * GG + T.gcell[bl]) * HW;
                float sum = 0.f;
                for (int s = 0; s < spp2; ++s) sum += bilinear(gather(T, bl * spp2 + s, plane));
                const float c = T.cnt[bl];
                const int64_t o = ((int64_t)n * a.D + d) * PP + bin0 + bl;
                out[o] = c > 0.f ? sum / c : 0.f;
                if (count) count[o] = c;
            }
        }
        __syncthreads();   // (the next tile overwrites the table)
    }
}

// grid: R * nc workgroups of kBwdGroups * kThreads lanes; workgroup (n, cls) owns the class's channels and its 2 * part * part
// cells of grad_trans.  Lane (grp, t) keeps table entries t, t + kThreads, ... and walks channels grp, grp + kBwdGroups, ...
// grad_in and grad_trans arrive zeroed.
__global__ __launch_bounds__(kBwdGroups * kThreads) void psroi_backward(
    const float *__restrict__ go, const float *__restrict__ in, const float *__restrict__ rois, const float *__restrict__ trans,
    const float *__restrict__ count, float *__restrict__ grad_in, float *__restrict__ grad_trans, PoolArgs a) {
    __shared__ Table T;
    __shared__ float sx[kTile], sy[kTile];
    constexpr int kLanes = kBwdGroups * kThreads;
    const int t = threadIdx.x % kThreads, grp = threadIdx.x / kThreads;
    const int cec = a.D / a.nc;
    const int cls = blockIdx.x % a.nc, n = blockIdx.x / a.nc;
    const Roi g = roi_geometry(rois, n, a);
    const int PP = a.P * a.P, spp2 = a.spp * a.spp, GG = a.G * a.G, part2 = a.part * a.part, bpt = kTile / spp2;
    const int64_t HW = (int64_t)a.H * a.W;
    const int64_t img = (int64_t)g.b * a.C * HW;

    for (int bin0 = 0; bin0 < PP; bin0 += bpt) {
        const int nb = min(bpt, PP - bin0);
        fill_table(T, g, trans, n, cls, bin0, nb, a);
        const int entries = nb * spp2;
        float ax[kPerLane], ay[kPerLane];
#pragma unroll
        for (int k = 0; k < kPerLane; ++k) ax[k] = ay[k] = 0.f;
        for (int dl = grp; dl < cec; dl += kBwdGroups) {
            const int d = cls * cec + dl;
#pragma unroll
            for (int k = 0; k < kPerLane; ++k) {
                const int e = t + k * kThreads;
                if (e >= entries) continue;
                const int bl = e / spp2;
                const int64_t o = ((int64_t)n * a.D + d) * PP + bin0 + bl;
                const int64_t poff = img + ((int64_t)d * GG + T.gcell[bl]) * HW;
                const Sample q = gather(T, e, in + poff);
                const float c = count[o];
                const bool ok = q.ok && c > 0.f;
                const float dv = ok ? go[o] / c : 0.f;
                if (ok) {
                    float *gp = grad_in + poff;
                    atomicAdd(gp + q.o00, (1.f - q.dx) * (1.f - q.dy) * dv);
                    atomicAdd(gp + q.o01, (1.f - q.dx) * q.dy * dv);
                    atomicAdd(gp + q.o10, q.dx * (1.f - q.dy) * dv);
                    atomicAdd(gp + q.o11, q.dx * q.dy * dv);
                }
                if (!a.no_trans) {
                    const float ddx = (q.v11 * q.dy + q.v10 * (1.f - q.dy) - q.v01 * q.dy - q.v00 * (1.f - q.dy)) * a.trans_std *
                                      dv * g.rw;
                    const float ddy = (q.v11 * q.dx + q.v01 * (1.f - q.dx) - q.v10 * q.dx - q.v00 * (1.f - q.dx)) * a.trans_std *
                                      dv * g.rh;
                    ax[k] += ok ? ddx : 0.f;
                    ay[k] += ok ? ddy : 0.f;
                }
            }
        }
        if (!a.no_trans) {
            for (int turn = 0; turn < kBwdGroups; ++turn) {   // the channel groups add their sums of an entry in group order
                if (grp == turn) {
#pragma unroll
                    for (int k = 0; k < kPerLane; ++k) {
                        const int e = t + k * kThreads;
                        if (e < entries) {
                            sx[e] = turn == 0 ? ax[k] : sx[e] + ax[k];
                            sy[e] = turn == 0 ? ay[k] : sy[e] + ay[k];
                        }
                    }
                }
                __syncthreads();
            }
            for (int bl = threadIdx.x; bl < nb; bl += kLanes) {   // a bin's samples, in sample order, into its first slot
                float bx = 0.f, by = 0.f;
                for (int s = 0; s < spp2; ++s) bx += sx[bl * spp2 + s], by += sy[bl * spp2 + s];
                sx[bl * spp2] = bx, sy[bl * spp2] = by;
            }
            __syncthreads();
            float *gt = grad_trans + ((int64_t)(n * a.nc + cls) * 2) * part2;
            for (int cell = threadIdx.x; cell < part2; cell += kLanes) {   // the bins of a part cell, in bin order
                float cx = 0.f, cy = 0.f;
                for (int bl = 0; bl < nb; ++bl)
                    if (T.pcell[bl] == cell) cx += sx[bl * spp2], cy += sy[bl * spp2];
                gt[cell] += cx;            // (this lane is the cell's only writer, in every tile)
                gt[part2 + cell] += cy;
            }
        }
        __syncthreads();
    }
}

int check_args(const char *what, const PoolArgs &a, int dtype) {
    if (dtype != EBFI_F32) return fail(EBFI_ERR_ARG, "%s: EBFI_F32 only (dtype %d)", what, dtype);
    if (a.B < 1 || a.C < 1 || a.H < 1 || a.W < 1 || a.R < 0 || a.nc < 1 || a.D < 1 || a.G < 1)
        return fail(EBFI_ERR_ARG, "%s: sizes must be >= 1 (B %d C %d H %d W %d R %d nc %d output_dim %d group_size %d)", what, a.B,
                    a.C, a.H, a.W, a.R, a.nc, a.D, a.G);
    if (a.P < 1 || a.part < 1 || a.spp < 1)
        return fail(EBFI_ERR_ARG, "%s: pooled_size %d, part_size %d and sample_per_part %d must be >= 1", what, a.P, a.part, a.spp);
    if (a.no_trans && a.nc != 1) return fail(EBFI_ERR_ARG, "%s: no_trans pools one class (nc %d)", what, a.nc);
    if ((int64_t)a.D * a.G * a.G != (int64_t)a.C)
        return fail(EBFI_ERR_ARG, "%s: input channels %d != output_dim %d * group_size %d^2", what, a.C, a.D, a.G);
    if (a.D % a.nc != 0) return fail(EBFI_ERR_ARG, "%s: output_dim %d is not a multiple of the %d classes of trans", what, a.D, a.nc);
    if (a.spp > kMaxSpp) return fail(EBFI_ERR_UNSUPPORTED, "%s: sample_per_part %d > %d", what, a.spp, kMaxSpp);
    if ((int64_t)a.H * a.W > INT_MAX || (int64_t)a.P * a.P > INT_MAX || (int64_t)a.part * a.part > INT_MAX)
        return fail(EBFI_ERR_UNSUPPORTED, "%s: H * W, pooled_size^2 and part_size^2 must stay below 2^31", what);
    return EBFI_OK;
}

}  // namespace

extern "C" int ebfi_dcn_pooling_forward(const void *input, const void *rois, const void *trans, void *output, void *count,
                                        int B, int C, int H, int W, int R, int nc, int no_trans, float spatial_scale,
                                        int output_dim, int group_size, int pooled_size, int part_size, int sample_per_part,
                                        float trans_std, int dtype, void *stream) {
    const PoolArgs a = {B, C, H, W, R, nc, no_trans ? 1 : 0, output_dim, group_size, pooled_size, part_size, sample_per_part,
                        spatial_scale, trans_std};
    const int rc = check_args("dcn_pooling_forward", a, dtype);
    if (rc != EBFI_OK) return rc;
    if (!input || !rois || !output || (!no_trans && !trans)) return fail(EBFI_ERR_ARG, "dcn_pooling_forward: null pointer");
    if (R == 0) return EBFI_OK;
    // enough workgroups to fill the card, at least 8 channels each: a chunk repeats the geometry of its (ROI, class)
    const int cec = output_dim / nc;
    const int64_t owners = (int64_t)R * nc;
    const int want = (int)std::min<int64_t>(cec, ceil_div(2048, owners));
    const int chunk_c = (int)std::max<int64_t>(ceil_div(cec, want), std::min(cec, 8));
    const int nchunk = (int)ceil_div(cec, chunk_c);
    if (owners * nchunk > INT_MAX) return fail(EBFI_ERR_UNSUPPORTED, "dcn_pooling_forward: launch grid beyond 2^31 - 1");
    hipStream_t st = static_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)(owners * nchunk)), block(kThreads);
    const double outs = (double)R * output_dim * pooled_size * pooled_size;
    {
        ProfScope ps_("psroi_forward", st, 0.0, ((double)B * C * H * W + outs * (count ? 2.0 : 1.0) + 5.0 * R) * 4.0);
        if (sample_per_part == 4)
            hipLaunchKernelGGL(psroi_forward<true>, grid, block, 0, st, (const float *)input, (const float *)rois,
                               (const float *)trans, (float *)output, (float *)count, a, nchunk, chunk_c);
        else
            hipLaunchKernelGGL(psroi_forward<false>, grid, block, 0, st, (const float *)input, (const float *)rois,
                               (const float *)trans, (float *)output, (float *)count, a, nchunk, chunk_c);
    }
    return check_launch("dcn_pooling_forward");
}

extern "C" int ebfi_dcn_pooling_backward(const void *grad_output, const void *input, const void *rois, const void *trans,
                                         const void *count, void *grad_input, void *grad_trans, int Rt, int B, int C, int H,
                                         int W, int R, int nc, int no_trans, float spatial_scale, int output_dim, int group_size,
                                         int pooled_size, int part_size, int sample_per_part, float trans_std, int dtype,
                                         void *stream) {
    const PoolArgs a = {B, C, H, W, R, nc, no_trans ? 1 : 0, output_dim, group_size, pooled_size, part_size, sample_per_part,
                        spatial_scale, trans_std};
    const int rc = check_args("dcn_pooling_backward", a, dtype);
    if (rc != EBFI_OK) return rc;
    if (!grad_output || !input || !rois || !count || !grad_input || (!no_trans && (!trans || !grad_trans)))
        return fail(EBFI_ERR_ARG, "dcn_pooling_backward: null pointer");
    if (!no_trans && Rt < R) return fail(EBFI_ERR_ARG, "dcn_pooling_backward: trans has %d rows for %d ROIs", Rt, R);
    if (R == 0) return EBFI_OK;
    if ((int64_t)R * nc > INT_MAX) return fail(EBFI_ERR_UNSUPPORTED, "dcn_pooling_backward: launch grid beyond 2^31 - 1");
    hipStream_t st = static_cast<hipStream_t>(stream);
    const size_t in_bytes = (size_t)B * C * H * W * sizeof(float);
    const size_t tr_bytes = no_trans ? 0 : (size_t)Rt * 2 * nc * part_size * part_size * sizeof(float);
    if (hipMemsetAsync(grad_input, 0, in_bytes, st) != hipSuccess ||
        (tr_bytes && hipMemsetAsync(grad_trans, 0, tr_bytes, st) != hipSuccess))
        return fail(EBFI_ERR_LAUNCH, "dcn_pooling_backward: memset of the gradients failed");
    const dim3 grid((unsigned)((int64_t)R * nc)), block(kBwdGroups * kThreads);
    const double outs = (double)R * output_dim * pooled_size * pooled_size;
    {
        ProfScope ps_("psroi_backward", st, 0.0, (double)in_bytes * 3.0 + (double)tr_bytes * 2.0 + (outs * 2.0 + 5.0 * R) * 4.0);
        hipLaunchKernelGGL(psroi_backward, grid, block, 0, st, (const float *)grad_output, (const float *)input,
                           (const float *)rois, (const float *)trans, (const float *)count, (float *)grad_input,
                           (float *)grad_trans, a);
    }
    return check_launch("dcn_pooling_backward");
}
