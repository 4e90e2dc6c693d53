// pack.hip -- packed rows of a ragged batch for gfx950: cloud after cloud, no pad row.
//
// A ragged batch is [B, N, .] with capacity N and n_valid[b] rows per cloud (include/pcl_hip.h, "ragged" entry points).  What runs
// once per raw point of PointNet++ part segmentation -- FP1, the head, the loss -- runs here on R = sum_b n_valid[b] rows [R, .]:
// row row_off[b] + i is point i of cloud b.  No reference counterpart (the reference resamples every cloud to one size).
//   row_offsets      exclusive scan of the clamped counts
//   fp_pack_rows     [onehot | skip | 3-NN interpolation] written straight as packed rows (three_interpolate + cat + drop pads)
//   fp_pack_rows_bwd its gradient w.r.t. points2 (atomics, as three_interp_bwd_kernel) and, on request, skip
//   pack / unpack    [B, N, W] <-> [R, W] in 32-bit words, the packed side through a column window of wider rows
// Every kernel clamps n_valid[b] to [1, N], touches no packed row >= n_rows and reads no pad row of a [B, N, .] operand.
#include "common.h"

namespace pcl {

constexpr int PK_T = 256;                      // threads per workgroup: four waves
constexpr int PK_ROWS = 16;                    // rows per workgroup of the FP kernels: one wave per row, four rows per wave
constexpr int PK_TILE = 64;                    // rows per workgroup of the generic pack / unpack

__device__ __forceinline__ int pk_count(const int32_t* __restrict__ n_valid, int b, int N) {
    return min(max(__builtin_amdgcn_readfirstlane(n_valid[b]), 1), N);
}

// row_off[b] = sum_{c < b} clamp(n_valid[c]); row_off[B] = R.  One workgroup (B <= 65535: at most 64 counts per thread).
__global__ __launch_bounds__(1024) void row_offsets_kernel(const int32_t* __restrict__ n_valid, int B, int N, int32_t* __restrict__ row_off) {
    __shared__ int part[1024];
    const int t = threadIdx.x;
    const int per = (B + 1023) / 1024;
    const int lo = min(t * per, B), hi = min(lo + per, B);
    int s = 0;
    for (int b = lo; b < hi; ++b) s += min(max(n_valid[b], 1), N);
    part[t] = s;
    __syncthreads();
    for (int off = 1; off < 1024; off <<= 1) {
        const int v = t >= off ? part[t - off] : 0;
        __syncthreads();
        part[t] += v;
        __syncthreads();
    }
    int run = part[t] - s;
    for (int b = lo; b < hi; ++b) { row_off[b] = run; run += min(max(n_valid[b], 1), N); }
    if (t == 1023) row_off[B] = part[1023];
}

// Grid (row tiles of N, B); a workgroup whose tile starts at or beyond n_b leaves before any load.  One wave per row: lanes 0 ..
// n_onehot + CS - 1 copy the row's head, then the wave walks the D2 interpolated columns -- VEC: 8-byte pieces (the block starts at
// byte 4 * (n_onehot + CS) of a 4 * ld byte row: 88 of 600 at FP1, 8-byte and not 16-byte aligned), else one float per lane.
// The sum is three_interp_kernel's: fl(fl(fl(p0 w0) + fl(p1 w1)) + fl(p2 w2)), so the rows equal three_interpolate + cat bit for bit.
// idx3 is clamped to [0, S) on load: a valid row's indices (pcl_three_nn_ragged_f32) are inside already, nothing can leave points2.
template <bool VEC>
__global__ __launch_bounds__(PK_T) void fp_pack_rows_kernel(const float* __restrict__ onehot, int n_onehot, const float* __restrict__ skip,
                                                            int CS, const float* __restrict__ points2, const int32_t* __restrict__ idx3,
                                                            const float* __restrict__ w3, const int32_t* __restrict__ n_valid,
                                                            const int32_t* __restrict__ row_off, int N, int S, int D2, int n_rows,
                                                            float* __restrict__ rows) {
    const int b = blockIdx.y, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int nb = pk_count(n_valid, b, N);
    const int i0 = blockIdx.x * PK_ROWS;
    if (i0 >= nb) return;
    const int r0 = __builtin_amdgcn_readfirstlane(row_off[b]);
    const int head = n_onehot + CS, ld = head + D2;
    const float* P2 = points2 + (size_t)b * S * D2;
    for (int i = i0 + wave; i < min(i0 + PK_ROWS, nb); i += PK_T / 64) {
        const int r = r0 + i;
        if (r < 0 || r >= n_rows) continue;                            // (a wrong n_rows / row_off stays inside the buffer)
        float* out = rows + (size_t)r * ld;
        for (int c = lane; c < head; c += 64)
            out[c] = c < n_onehot ? onehot[(size_t)b * n_onehot + c] : skip[((size_t)b * N + i) * CS + (c - n_onehot)];
        out += head;
        if (S == 1) {                                                  // one source: its row, untouched (the reference's expand)
            if constexpr (VEC) {
                for (int c = 2 * lane; c < D2; c += 128) *reinterpret_cast<float2*>(out + c) = *reinterpret_cast<const float2*>(P2 + c);
            } else {
                for (int c = lane; c < D2; c += 64) out[c] = P2[c];
            }
            continue;
        }
        const int32_t* ii = idx3 + ((size_t)b * N + i) * 3;
        const float* ww = w3 + ((size_t)b * N + i) * 3;
        const float* a0 = P2 + (size_t)min(max(ii[0], 0), S - 1) * D2;
        const float* a1 = P2 + (size_t)min(max(ii[1], 0), S - 1) * D2;
        const float* a2 = P2 + (size_t)min(max(ii[2], 0), S - 1) * D2;
        const float w0 = ww[0], w1 = ww[1], w2 = ww[2];
        if constexpr (VEC) {
            for (int c = 2 * lane; c < D2; c += 128) {
                const float2 p0 = *reinterpret_cast<const float2*>(a0 + c), p1 = *reinterpret_cast<const float2*>(a1 + c);
                const float2 p2 = *reinterpret_cast<const float2*>(a2 + c);
                float2 o;
                o.x = __fadd_rn(__fadd_rn(__fmul_rn(p0.x, w0), __fmul_rn(p1.x, w1)), __fmul_rn(p2.x, w2));
                o.y = __fadd_rn(__fadd_rn(__fmul_rn(p0.y, w0), __fmul_rn(p1.y, w1)), __fmul_rn(p2.y, w2));
                *reinterpret_cast<float2*>(out + c) = o;
            }
        } else {
            for (int c = lane; c < D2; c += 64)
                out[c] = __fadd_rn(__fadd_rn(__fmul_rn(a0[c], w0), __fmul_rn(a1[c], w1)), __fmul_rn(a2[c], w2));
        }
    }
}

// gpoints2[b, idx3[b,i,k], :] += w3[b,i,k] * grows[row_off[b] + i, head:]  (gpoints2 zero-filled by the launcher).  Same grid; one
// wave per row, and each atomic wave-instruction adds 64 consecutive floats of ONE gpoints2 row (256 contiguous bytes).
__global__ __launch_bounds__(PK_T) void fp_pack_rows_bwd_kernel(const float* __restrict__ grows, int head, const int32_t* __restrict__ idx3,
                                                                const float* __restrict__ w3, const int32_t* __restrict__ n_valid,
                                                                const int32_t* __restrict__ row_off, int N, int S, int D2, int n_rows,
                                                                float* __restrict__ gp2) {
    const int b = blockIdx.y, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int nb = pk_count(n_valid, b, N);
    const int i0 = blockIdx.x * PK_ROWS;
    if (i0 >= nb) return;
    const int r0 = __builtin_amdgcn_readfirstlane(row_off[b]);
    const int ld = head + D2;
    float* G2 = gp2 + (size_t)b * S * D2;
    for (int i = i0 + wave; i < min(i0 + PK_ROWS, nb); i += PK_T / 64) {
        const int r = r0 + i;
        if (r < 0 || r >= n_rows) continue;
        const float* g = grows + (size_t)r * ld + head;
        const int32_t* ii = idx3 + ((size_t)b * N + i) * 3;
        const float* ww = w3 + ((size_t)b * N + i) * 3;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            float* dst = G2 + (size_t)min(max(ii[k], 0), S - 1) * D2;
            const float w = ww[k];
            for (int c = lane; c < D2; c += 64) unsafeAtomicAdd(dst + c, __fmul_rn(g[c], w));
        }
    }
}

// S == 1: gpoints2[b, 0, c] = sum_{i < n_b} grows[row_off[b] + i, head + c] without atomics.  Grid (column tiles of 64, B); thread
// (column, q) adds the rows i = q, q + 4, ... in ascending order, the four partial sums are added in q order: run-to-run identical.
__global__ __launch_bounds__(PK_T) void fp_pack_rows_bwd_one_kernel(const float* __restrict__ grows, int head, const int32_t* __restrict__ n_valid,
                                                                    const int32_t* __restrict__ row_off, int N, int D2, int n_rows,
                                                                    float* __restrict__ gp2) {
    __shared__ float part[PK_T];
    const int b = blockIdx.y, q = threadIdx.x >> 6, c = blockIdx.x * 64 + (threadIdx.x & 63);
    const int nb = pk_count(n_valid, b, N);
    const int r0 = __builtin_amdgcn_readfirstlane(row_off[b]);
    const int ld = head + D2;
    float s = 0.f;
    if (c < D2)
        for (int i = q; i < nb; i += PK_T / 64) {
            const int r = r0 + i;
            if (r >= 0 && r < n_rows) s = __fadd_rn(s, grows[(size_t)r * ld + head + c]);
        }
    part[threadIdx.x] = s;
    __syncthreads();
    if (q == 0 && c < D2) {
        const int t = threadIdx.x;
        gp2[(size_t)b * D2 + c] = __fadd_rn(__fadd_rn(__fadd_rn(part[t], part[t + 64]), part[t + 128]), part[t + 192]);
    }
}

// Generic rows of W 32-bit words.  PACK: packed[(row_off[b] + i) * ld + col0 + c] = dense[(b N + i) W + c] for i < n_b.  Unpack: the
// other direction, and the pad rows of dense are written as zero bits.  Grid (tiles of PK_TILE rows, B); the tile is walked as
// one flat run of words, so consecutive lanes touch consecutive words of the dense side.
template <bool PACK>
__global__ __launch_bounds__(PK_T) void pack_rows_kernel(const uint32_t* __restrict__ src, const int32_t* __restrict__ n_valid,
                                                         const int32_t* __restrict__ row_off, int N, int W, int ld, int col0, int n_rows,
                                                         uint32_t* __restrict__ dst) {
    const int b = blockIdx.y;
    const int nb = pk_count(n_valid, b, N);
    const int i0 = blockIdx.x * PK_TILE;
    if (PACK && i0 >= nb) return;
    const int r0 = __builtin_amdgcn_readfirstlane(row_off[b]);
    const int rows_here = min(PK_TILE, N - i0);
    for (int e = threadIdx.x; e < rows_here * W; e += PK_T) {
        const int k = e / W, c = e - k * W, i = i0 + k;
        const int r = r0 + i;
        const bool live = i < nb && r >= 0 && r < n_rows;
        const size_t dense = ((size_t)b * N + i) * W + c, packed = (size_t)r * ld + col0 + c;
        if constexpr (PACK) {
            if (live) dst[packed] = src[dense];
        } else {
            dst[dense] = live ? src[packed] : 0u;
        }
    }
}

}  // namespace pcl
using namespace pcl;

static inline bool aligned8(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 7) == 0; }

extern "C" int pcl_row_offsets_i32(const int32_t* n_valid, int B, int N, int32_t* row_off, void* stream) {
    PCL_REQUIRE(n_valid && row_off, "pcl_row_offsets_i32: null pointer");
    PCL_REQUIRE(B >= 1 && B <= 65535 && N >= 1 && (long long)B * N < 2147483647LL, "pcl_row_offsets_i32: bad sizes B=%d N=%d", B, N);
    hipLaunchKernelGGL(row_offsets_kernel, dim3(1), dim3(1024), 0, as_stream(stream), n_valid, B, N, row_off);
    return check_launch("pcl_row_offsets_i32");
}

static int pack_sizes_ok(const char* who, int B, int N, int n_rows) {
    PCL_REQUIRE(B >= 0 && B <= 65535 && N >= 0, "%s: bad sizes B=%d N=%d (B <= 65535: grid.y)", who, B, N);
    PCL_REQUIRE(n_rows >= 0 && (long long)n_rows <= (long long)B * N, "%s: n_rows=%d outside [0, B*N]", who, n_rows);
    return PCL_OK;
}

extern "C" int pcl_fp_pack_rows_f32(const float* onehot, int n_onehot, const float* skip, int CS, const float* points2,
                                    const int32_t* idx3, const float* w3, const int32_t* n_valid, const int32_t* row_off, int B, int N,
                                    int S, int D2, int n_rows, float* rows, void* stream) {
    const char* who = "pcl_fp_pack_rows_f32";
    PCL_REQUIRE(points2 && n_valid && row_off && rows, "%s: null pointer", who);
    PCL_REQUIRE(S >= 1 && D2 >= 1 && n_onehot >= 0 && CS >= 0, "%s: bad sizes S=%d D2=%d n_onehot=%d CS=%d", who, S, D2, n_onehot, CS);
    PCL_REQUIRE(n_onehot == 0 || onehot, "%s: null pointer (onehot, n_onehot=%d)", who, n_onehot);
    PCL_REQUIRE(CS == 0 || skip, "%s: null pointer (skip, CS=%d)", who, CS);
    PCL_REQUIRE(S == 1 || (idx3 && w3), "%s: null pointer (idx3 / w3 with S=%d)", who, S);
    if (int rc = pack_sizes_ok(who, B, N, n_rows)) return rc;
    if (B == 0 || N == 0 || n_rows == 0) return PCL_OK;
    const dim3 grid((N + PK_ROWS - 1) / PK_ROWS, B);
    const bool vec = D2 % 2 == 0 && (n_onehot + CS) % 2 == 0 && aligned8(points2) && aligned8(rows);
    if (vec)
        hipLaunchKernelGGL(fp_pack_rows_kernel<true>, grid, dim3(PK_T), 0, as_stream(stream), onehot, n_onehot, skip, CS, points2, idx3, w3,
                           n_valid, row_off, N, S, D2, n_rows, rows);
    else
        hipLaunchKernelGGL(fp_pack_rows_kernel<false>, grid, dim3(PK_T), 0, as_stream(stream), onehot, n_onehot, skip, CS, points2, idx3, w3,
                           n_valid, row_off, N, S, D2, n_rows, rows);
    return check_launch(who);
}

static int pack_rows_run(const char* who, bool pack, const void* src, const int32_t* n_valid, const int32_t* row_off, int B, int N, int W,
                         int ld, int col0, int n_rows, void* dst, void* stream) {
    PCL_REQUIRE(src && n_valid && row_off && dst, "%s: null pointer", who);
    PCL_REQUIRE(W >= 1 && col0 >= 0 && ld >= 1 && (long long)col0 + W <= ld, "%s: bad window W=%d col0=%d ld=%d", who, W, col0, ld);
    PCL_REQUIRE((long long)PK_TILE * W < 2147483647LL, "%s: W=%d too wide", who, W);
    if (int rc = pack_sizes_ok(who, B, N, n_rows)) return rc;
    if (B == 0 || N == 0) return PCL_OK;
    const dim3 grid((N + PK_TILE - 1) / PK_TILE, B);
    if (pack)
        hipLaunchKernelGGL(pack_rows_kernel<true>, grid, dim3(PK_T), 0, as_stream(stream), static_cast<const uint32_t*>(src), n_valid,
                           row_off, N, W, ld, col0, n_rows, static_cast<uint32_t*>(dst));
    else
        hipLaunchKernelGGL(pack_rows_kernel<false>, grid, dim3(PK_T), 0, as_stream(stream), static_cast<const uint32_t*>(src), n_valid,
                           row_off, N, W, ld, col0, n_rows, static_cast<uint32_t*>(dst));
    return check_launch(who);
}

extern "C" int pcl_pack_rows_b32(const void* src, const int32_t* n_valid, const int32_t* row_off, int B, int N, int W, int ld, int col0,
                                 int n_rows, void* dst, void* stream) {
    return pack_rows_run("pcl_pack_rows_b32", true, src, n_valid, row_off, B, N, W, ld, col0, n_rows, dst, stream);
}

extern "C" int pcl_unpack_rows_b32(const void* src, const int32_t* n_valid, const int32_t* row_off, int B, int N, int W, int ld, int col0,
                                   int n_rows, void* dst, void* stream) {
    return pack_rows_run("pcl_unpack_rows_b32", false, src, n_valid, row_off, B, N, W, ld, col0, n_rows, dst, stream);
}

extern "C" int pcl_fp_pack_rows_bwd_f32(const float* grows, int n_onehot, int CS, const int32_t* idx3, const float* w3,
                                        const int32_t* n_valid, const int32_t* row_off, int B, int N, int S, int D2, int n_rows,
                                        float* gpoints2, float* gskip, void* stream) {
    const char* who = "pcl_fp_pack_rows_bwd_f32";
    PCL_REQUIRE(grows && n_valid && row_off && gpoints2, "%s: null pointer", who);
    PCL_REQUIRE(S >= 1 && D2 >= 1 && n_onehot >= 0 && CS >= 0, "%s: bad sizes S=%d D2=%d n_onehot=%d CS=%d", who, S, D2, n_onehot, CS);
    PCL_REQUIRE(S == 1 || (idx3 && w3), "%s: null pointer (idx3 / w3 with S=%d)", who, S);
    PCL_REQUIRE(!gskip || CS > 0, "%s: gskip given with CS=0", who);
    if (int rc = pack_sizes_ok(who, B, N, n_rows)) return rc;
    if (B == 0) return PCL_OK;
    hipStream_t st = as_stream(stream);
    const int head = n_onehot + CS;
    if (S == 1) {
        if (N == 0) {
            hipError_t e = hipMemsetAsync(gpoints2, 0, sizeof(float) * (size_t)B * D2, st);
            if (e != hipSuccess) return fail(PCL_EHIP, "%s: memset: %s", who, hipGetErrorString(e));
            return PCL_OK;
        }
        hipLaunchKernelGGL(fp_pack_rows_bwd_one_kernel, dim3((D2 + 63) / 64, B), dim3(PK_T), 0, st, grows, head, n_valid, row_off, N, D2,
                           n_rows, gpoints2);
    } else {
        hipError_t e = hipMemsetAsync(gpoints2, 0, sizeof(float) * (size_t)B * S * D2, st);
        if (e != hipSuccess) return fail(PCL_EHIP, "%s: memset: %s", who, hipGetErrorString(e));
        if (N == 0 || n_rows == 0) return PCL_OK;
        hipLaunchKernelGGL(fp_pack_rows_bwd_kernel, dim3((N + PK_ROWS - 1) / PK_ROWS, B), dim3(PK_T), 0, st, grows, head, idx3, w3, n_valid,
                           row_off, N, S, D2, n_rows, gpoints2);
    }
    if (int rc = check_launch(who)) return rc;
    if (gskip && N > 0)
        return pack_rows_run(who, false, grows, n_valid, row_off, B, N, CS, head + D2, n_onehot, n_rows, gskip, stream);
    return PCL_OK;
}
