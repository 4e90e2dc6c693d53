// segpool.hip -- pooling over the clouds of packed rows for gfx950.
//
// Packed rows are section 15's (pack.hip): row_off int32 [B+1] from pcl_row_offsets_i32, cloud b owns the packed rows
// row_off[b] .. row_off[b+1] - 1 of an [n_rows, C] matrix.  What PointNet and its T-Nets do per cloud on such rows:
//   row_cloud        row_cloud[r] = the cloud that owns packed row r (made once per batch; read by the two kernels that walk rows)
//   bn_act_seg_max   out[b, c] = max over the cloud's rows of lrelu(fmaf(scale[c], y, shift[c]), slope), arg = the first such row
//   .. _bwd          du = act' * (the winner's gmax, else 0) and the BatchNorm-backward sums (sum du, sum du*y) as fp64 partial rows
//   seg_broadcast    dst[r] = src[row_cloud[r]]: a per-cloud vector onto the cloud's rows
//   seg_sum          its gradient: per-cloud column sums, fp64 in a fixed order
// No reference counterpart (the reference resamples every cloud to one size and pools over a dense axis).  Every kernel clamps what
// it reads from row_off / row_cloud, touches no packed row >= n_rows and uses plain vector stores: no atomics.
#include "common.h"

namespace pcl {

constexpr int SP_STAT_ROWS = 1024;             // rows of a stats workspace (mlp.hip: STAT_ROWS)

__device__ __forceinline__ float sp_lrelu(float x, float slope) { return x > 0.f ? x : x * slope; }      // mlp.hip: lrelu

// the rows [lo, hi) of cloud b that exist in the buffer, and the cloud's first row r0 (arg counts from it)
__device__ __forceinline__ void sp_segment(const int32_t* __restrict__ row_off, int b, int n_rows, int& r0, int& lo, int& hi) {
    r0 = __builtin_amdgcn_readfirstlane(row_off[b]);
    const int r1 = __builtin_amdgcn_readfirstlane(row_off[b + 1]);
    lo = max(r0, 0);
    hi = min(r1, n_rows);
}

// One thread per packed row: the last b in [0, B) with row_off[b] <= r (a binary search of at most 16 steps, once per batch).
__global__ __launch_bounds__(256) void row_cloud_kernel(const int32_t* __restrict__ row_off, int B, int n_rows,
                                                        int32_t* __restrict__ row_cloud) {
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= n_rows) return;
    int lo = 0, hi = B - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (row_off[mid] <= r) lo = mid; else hi = mid - 1;
    }
    row_cloud[r] = lo;
}

// The better of two (value, row) candidates: the larger value, and of equal values the smaller row -- the result of the sequential
// scan whatever the order of the folds (bn_act_maxmean_sliced_kernel's rule).
__device__ __forceinline__ void sp_take(float& best, int& bi, float z, int s) {
    if (z > best || (z == best && s < bi)) { best = z; bi = s; }
}

// Grid (channel tiles of 64, B), 64 * SL threads.  A workgroup owns 64 channels of one cloud; its rows are dealt to slices
// (slice j takes rows j, j + n_slices, ...), a slice keeps the first row that attains its maximum (strict >), and the slices are
// folded with sp_take.  VEC (C % 4 == 0, 16-byte aligned Y): a lane moves a float4 -- 16 lanes cover the 64 channels, so a wave is
// 4 slices (n_slices = 4 SL) folded through two lane exchanges; otherwise a lane is one channel and a wave one slice.
template <int SL, bool VEC>
__global__ __launch_bounds__(64 * SL) void bn_act_seg_max_kernel(const float* __restrict__ Y, const int32_t* __restrict__ row_off,
                                                                 const float* __restrict__ scale, const float* __restrict__ shift,
                                                                 float slope, int C, int n_rows, float* __restrict__ out,
                                                                 int32_t* __restrict__ arg) {
    __shared__ float sz[SL][64];
    __shared__ int ss[SL][64];
    const int lane = threadIdx.x & 63, sl = threadIdx.x >> 6;
    const int b = blockIdx.y, c0 = blockIdx.x * 64;
    int r0, lo, hi;
    sp_segment(row_off, b, n_rows, r0, lo, hi);
    if constexpr (VEC) {
        const int q = lane >> 4, c = c0 + 4 * (lane & 15);
        float best[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
        int bi[4] = {0, 0, 0, 0};
        if (c < C) {                                                   // (C % 4 == 0: the whole float4 is inside)
            const float4 a = *reinterpret_cast<const float4*>(scale + c), h = *reinterpret_cast<const float4*>(shift + c);
            for (int r = lo + sl * 4 + q; r < hi; r += 4 * SL) {
                const float4 y = *reinterpret_cast<const float4*>(Y + (size_t)r * C + c);
                const int s = r - r0;
                const float z0 = sp_lrelu(fmaf(a.x, y.x, h.x), slope), z1 = sp_lrelu(fmaf(a.y, y.y, h.y), slope);
                const float z2 = sp_lrelu(fmaf(a.z, y.z, h.z), slope), z3 = sp_lrelu(fmaf(a.w, y.w, h.w), slope);
                if (z0 > best[0]) { best[0] = z0; bi[0] = s; }
                if (z1 > best[1]) { best[1] = z1; bi[1] = s; }
                if (z2 > best[2]) { best[2] = z2; bi[2] = s; }
                if (z3 > best[3]) { best[3] = z3; bi[3] = s; }
            }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
#pragma unroll
            for (int m = 16; m <= 32; m <<= 1) {
                const float z = __shfl_xor(best[j], m, 64);
                const int s = __shfl_xor(bi[j], m, 64);
                sp_take(best[j], bi[j], z, s);
            }
        }
        if (q == 0) {
#pragma unroll
            for (int j = 0; j < 4; ++j) { sz[sl][4 * lane + j] = best[j]; ss[sl][4 * lane + j] = bi[j]; }
        }
    } else {
        const int c = c0 + lane;
        float best = -INFINITY;
        int bi = 0;
        if (c < C) {
            const float a = scale[c], h = shift[c];
            for (int r = lo + sl; r < hi; r += SL) {
                const float z = sp_lrelu(fmaf(a, Y[(size_t)r * C + c], h), slope);
                if (z > best) { best = z; bi = r - r0; }
            }
        }
        sz[sl][lane] = best; ss[sl][lane] = bi;
    }
    __syncthreads();
    const int c = c0 + lane;
    if (sl != 0 || c >= C) return;
    float best = sz[0][lane];
    int bi = ss[0][lane];
#pragma unroll
    for (int j = 1; j < SL; ++j) sp_take(best, bi, sz[j][lane], ss[j][lane]);
    out[(size_t)b * C + c] = best;
    arg[(size_t)b * C + c] = bi;
}

// bn_act_maxmean_bwd_kernel (mlp.hip) on packed rows, without the mean's share: grid (channel blocks of CW, <= 1024 row slices),
// CW = min(256, next power of two >= C) lanes over the channels and 256 / CW rows per pass; workgroup y leaves its fp64 partial
// (sum du, sum du*y) as row y of stats [rows][2][C].  The cloud of a row comes from row_cloud, clamped to [0, B).
__global__ __launch_bounds__(256) void bn_act_seg_max_bwd_kernel(const float* __restrict__ gmax, int ldg, const int32_t* __restrict__ arg,
                                                                 const float* __restrict__ Y, const float* __restrict__ scale,
                                                                 const float* __restrict__ shift, float slope,
                                                                 const int32_t* __restrict__ row_off, const int32_t* __restrict__ row_cloud,
                                                                 int B, int C, int CW, int n_rows, float* __restrict__ du,
                                                                 double* __restrict__ stats) {
    __shared__ double red[2 * 256];
    const int RS = 256 / CW, rsub = threadIdx.x / CW, cw = threadIdx.x % CW;
    const int c = blockIdx.x * CW + cw;
    double s1 = 0.0, s2 = 0.0;
    if (c < C) {
        const float a = scale[c], h = shift[c];
        for (int r = blockIdx.y * RS + rsub; r < n_rows; r += gridDim.y * RS) {
            const int b = min(max(row_cloud[r], 0), B - 1);
            const int srow = r - row_off[b];
            const size_t e = (size_t)r * C + c;
            const float y = Y[e];
            const float gz = arg[(size_t)b * C + c] == srow ? gmax[(size_t)b * ldg + c] : 0.f;
            const float v = gz * (fmaf(a, y, h) > 0.f ? 1.f : slope);
            du[e] = v;
            s1 += v; s2 += (double)v * y;
        }
    }
    if (RS > 1) {                                                      // fold the row-lanes of the block (mlp.hip: fold_row_lanes)
        red[rsub * CW + cw] = s1;
        red[(RS + rsub) * CW + cw] = s2;
        __syncthreads();
        if (rsub == 0)
            for (int j = 1; j < RS; ++j) { s1 += red[j * CW + cw]; s2 += red[(RS + j) * CW + cw]; }
    }
    if (rsub == 0 && c < C) {
        double* dst = stats + (size_t)blockIdx.y * 2 * C;
        dst[c] = s1; dst[C + c] = s2;
    }
}

// dst[r, :] = src[row_cloud[r], :] as one flat run of pieces (float4 when VEC: C % 4 == 0 and both sides 16-byte aligned).
template <bool VEC>
__global__ __launch_bounds__(256) void seg_broadcast_kernel(const float* __restrict__ src, const int32_t* __restrict__ row_cloud, int B,
                                                            int C, size_t total, float* __restrict__ dst) {
    const int W = VEC ? C / 4 : C;                                     // pieces per row; total = n_rows * W
    for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (size_t)gridDim.x * 256) {
        const int r = (int)(e / W), k = (int)(e - (size_t)r * W);
        const int b = min(max(row_cloud[r], 0), B - 1);
        if constexpr (VEC) reinterpret_cast<float4*>(dst)[e] = reinterpret_cast<const float4*>(src)[(size_t)b * W + k];
        else dst[e] = src[(size_t)b * W + k];
    }
}

// gsrc[b, c] = sum over the cloud's rows of g[r, c].  Grid (channel tiles of 64, B), 64 * SL threads: slice j adds its rows
// j, j + SL, ... in ascending order in fp64, wave 0 adds the SL partial sums in slice order and rounds once: a fixed order.
template <int SL>
__global__ __launch_bounds__(64 * SL) void seg_sum_kernel(const float* __restrict__ g, const int32_t* __restrict__ row_off, int C,
                                                          int n_rows, float* __restrict__ gsrc) {
    __shared__ double sm[SL][64];
    const int lane = threadIdx.x & 63, sl = threadIdx.x >> 6;
    const int b = blockIdx.y, c = blockIdx.x * 64 + lane;
    int r0, lo, hi;
    sp_segment(row_off, b, n_rows, r0, lo, hi);
    double s = 0.0;
    if (c < C)
        for (int r = lo + sl; r < hi; r += SL) s += (double)g[(size_t)r * C + c];
    sm[sl][lane] = s;
    __syncthreads();
    if (sl != 0 || c >= C) return;
#pragma unroll
    for (int j = 1; j < SL; ++j) s += sm[j][lane];
    gsrc[(size_t)b * C + c] = (float)s;
}

}  // namespace pcl
using namespace pcl;


static int seg_sizes_ok(const char* who, int B, int C, int n_rows) {
    PCL_REQUIRE(B >= 1 && B <= 65535 && C >= 1, "%s: bad sizes B=%d C=%d (1 <= B <= 65535: grid.y)", who, B, C);
    PCL_REQUIRE(n_rows >= 0, "%s: n_rows=%d is negative", who, n_rows);
    return PCL_OK;
}

extern "C" int pcl_row_cloud_i32(const int32_t* row_off, int B, int n_rows, int32_t* row_cloud, void* stream) {
    const char* who = "pcl_row_cloud_i32";
    PCL_REQUIRE(row_off && row_cloud, "%s: null pointer", who);
    if (int rc = seg_sizes_ok(who, B, 1, n_rows)) return rc;
    if (n_rows == 0) return PCL_OK;
    hipLaunchKernelGGL(row_cloud_kernel, dim3((n_rows + 255) / 256), dim3(256), 0, as_stream(stream), row_off, B, n_rows, row_cloud);
    return check_launch(who);
}

extern "C" int pcl_bn_act_seg_max_f32(const float* Y, const int32_t* row_off, const float* scale, const float* shift, float slope, int B,
                                      int C, int n_rows, float* out, int32_t* arg, void* stream) {
    const char* who = "pcl_bn_act_seg_max_f32";
    PCL_REQUIRE(Y && row_off && scale && shift && out && arg, "%s: null pointer", who);
    if (int rc = seg_sizes_ok(who, B, C, n_rows)) return rc;
    const dim3 grid((C + 63) / 64, B);
    const bool vec = C % 4 == 0 && al16(Y, scale, shift);
    const bool wide = n_rows / B >= 256;                               // the mean cloud: 16 waves per workgroup, else 4
    hipStream_t st = as_stream(stream);
#define SP_MAX(SL, VEC) hipLaunchKernelGGL((bn_act_seg_max_kernel<SL, VEC>), grid, dim3(64 * SL), 0, st, Y, row_off, scale, shift, slope, C, n_rows, out, arg)
    if (wide) { if (vec) SP_MAX(16, true); else SP_MAX(16, false); }
    else { if (vec) SP_MAX(4, true); else SP_MAX(4, false); }
#undef SP_MAX
    return check_launch(who);
}

extern "C" int pcl_bn_act_seg_max_bwd_f32(const float* gmax, int ldg, const int32_t* arg, const float* Y, const float* scale,
                                          const float* shift, float slope, const int32_t* row_off, const int32_t* row_cloud, int B, int C,
                                          int n_rows, float* du, double* stats_ws, int* stat_rows_out, void* stream) {
    const char* who = "pcl_bn_act_seg_max_bwd_f32";
    PCL_REQUIRE(gmax && arg && Y && scale && shift && row_off && row_cloud && du && stats_ws && stat_rows_out, "%s: null pointer", who);
    if (int rc = seg_sizes_ok(who, B, C, n_rows)) return rc;
    PCL_REQUIRE(ldg >= C, "%s: gmax row stride ldg=%d below the width C=%d", who, ldg, C);
    int CW = 256;
    while (CW / 2 >= C && CW > 1) CW >>= 1;
    const int RS = 256 / CW;
    int rows = (n_rows + RS - 1) / RS;
    rows = rows < 1 ? 1 : (rows < SP_STAT_ROWS ? rows : SP_STAT_ROWS);  // (n_rows == 0: one row of zero sums)
    *stat_rows_out = rows;
    hipLaunchKernelGGL(bn_act_seg_max_bwd_kernel, dim3((C + CW - 1) / CW, rows), dim3(256), 0, as_stream(stream), gmax, ldg, arg, Y, scale,
                       shift, slope, row_off, row_cloud, B, C, CW, n_rows, du, stats_ws);
    return check_launch(who);
}

extern "C" int pcl_seg_broadcast_rows_f32(const float* src, const int32_t* row_cloud, int B, int C, int n_rows, float* dst, void* stream) {
    const char* who = "pcl_seg_broadcast_rows_f32";
    PCL_REQUIRE(src && row_cloud && dst, "%s: null pointer", who);
    if (int rc = seg_sizes_ok(who, B, C, n_rows)) return rc;
    if (n_rows == 0) return PCL_OK;
    const bool vec = C % 4 == 0 && al16(src, dst);
    const size_t total = (size_t)n_rows * (vec ? C / 4 : C);
    const int blocks = (int)((total + 255) / 256 < 8192 ? (total + 255) / 256 : 8192);
    if (vec) hipLaunchKernelGGL(seg_broadcast_kernel<true>, dim3(blocks), dim3(256), 0, as_stream(stream), src, row_cloud, B, C, total, dst);
    else hipLaunchKernelGGL(seg_broadcast_kernel<false>, dim3(blocks), dim3(256), 0, as_stream(stream), src, row_cloud, B, C, total, dst);
    return check_launch(who);
}

extern "C" int pcl_seg_sum_rows_f32(const float* g, const int32_t* row_off, int B, int C, int n_rows, float* gsrc, void* stream) {
    const char* who = "pcl_seg_sum_rows_f32";
    PCL_REQUIRE(g && row_off && gsrc, "%s: null pointer", who);
    if (int rc = seg_sizes_ok(who, B, C, n_rows)) return rc;
    const dim3 grid((C + 63) / 64, B);
    if (n_rows / B >= 256) hipLaunchKernelGGL(seg_sum_kernel<16>, grid, dim3(1024), 0, as_stream(stream), g, row_off, C, n_rows, gsrc);
    else hipLaunchKernelGGL(seg_sum_kernel<4>, grid, dim3(256), 0, as_stream(stream), g, row_off, C, n_rows, gsrc);
    return check_launch(who);
}
