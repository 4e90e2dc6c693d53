// infer_mfma.h -- the tile pieces shared by the frozen-inference kernels (infer.hip, infer_fp.hip, infer_pointnet.hip,
// infer_pointnet_seg.hip): the sizes of a tile, the MFMA layer steps and the accumulator-to-row map (acc_row), and on top of
// them one LDS-to-LDS layer (tile_layer), the last layer under a max (max_passes), the K = 3 points layer (points_layer), the
// tile-of-one-cloud prologue (cloud_tile) and the per-cloud tile-max kernel (tile_max_kernel).  tile_layer, max_passes and
// points_layer are one body each for fp32 and bf16 tiles, selected by the tile's element type.  What the kernels' headers promise
// is held here once: rows of a tile are independent (a pad row's contents stay in that row), pad rows are selected out under a
// max, and a value is the same chain of operations in every kernel that calls a piece.
//
// A workgroup of 4 waves holds a 64-row tile of activations in LDS (row stride LDX).  Wave w owns the 32-column blocks
// w, w+4, ... of both 32-row blocks and accumulates them on v_mfma_f32_32x32x2_f32: A from LDS (ds_read_b128), B straight
// from the weight matrix in L2 (one 16-byte load per lane per 4 k-steps).  The k order inside a block of 8 is permuted
// (lane half h holds k = 8q + 4h + i at k-step 4q + i) identically for A and B, so each lane moves 16-byte pieces; the sum
// is the same set of products in a different order.  Accumulator element r of lane (lr, lh) is row acc_row(rb, r, lh),
// column cb*32 + lr.
//
// mfma_layer_bf16 is the same step with bf16 operands (v_mfma_f32_32x32x16_bf16, fp32 accumulation): the tile and the weight
// matrix hold bf16, lane (lr, lh) takes A[row lr][k = 16q + 8lh + j] and W[col lr][k = 16q + 8lh + j], j < 8, as one 16-byte
// piece each at k-block q; the k-blocks run in ascending order and no k permutation is needed.  Same ownership, same
// accumulator map.  LDX = K + row_pad<__bf16>: rows of (2K + 16) bytes, an odd number of 16-byte pieces, so the 16-byte reads of
// consecutive rows fall on distinct banks, and every row stays 16-byte aligned.
#pragma once
#include <type_traits>

#include "common.h"

namespace pcl {
namespace infer {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));

constexpr int NT = 256;                    // threads per workgroup (4 waves)
constexpr int RT = 64;                     // rows per tile (two 32-row MFMA blocks)
// a tile's row stride is its width + one 16-byte piece (4 floats / 8 bf16): ds_read_b128 rows on distinct banks
template <typename XT>
constexpr int row_pad = 16 / sizeof(XT);
constexpr int LD128 = 128 + row_pad<float>;        // row stride of a 128-wide fp32 tile
constexpr int MAX_NJ = 2;                  // the last layer under a max: column blocks per wave and pass (64 accumulator registers)
constexpr int MAX_PASS = 4 * MAX_NJ * 32;  // ... and columns per pass (256)

__host__ __device__ constexpr int imax(int a, int b) { return a > b ? a : b; }

__device__ __forceinline__ float act(float u, float slope) { return u > 0.f ? u : u * slope; }

// the tile row of accumulator element r of 32-row block rb in lane half lh
__device__ __forceinline__ int acc_row(int rb, int r, int lh) { return rb * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh; }

template <int NRB, int NJ>
__device__ __forceinline__ void acc_clear(f32x16 (&acc)[NRB][NJ]) {
#pragma unroll
    for (int rb = 0; rb < NRB; ++rb)
#pragma unroll
        for (int j = 0; j < NJ; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[rb][j][r] = 0.f;
}

// acc[rb][j] += X[rb*32 + row][k] * W[(w + 4j)*32 + col][k] over k < K; acc is NOT cleared.  X in LDS with row stride LDX; W has
// row stride ldw -- the tile may hold columns [k0, k0 + K) of a wider input, W then points at column k0 of a [*, ldw] matrix
// (16-byte aligned there).  Chunks accumulated in ascending order give one fp32 chain per element in the k order of mfma_layer over
// the whole width.
template <int K, int LDX, int NJ, int NCB>
__device__ __forceinline__ void mfma_layer_acc(const float* __restrict__ X, const float* __restrict__ W, int ldw, int wave, int lane,
                                               f32x16 (&acc)[2][NJ]) {
    const int lr = lane & 31, lh = lane >> 5;
    const float* xa0 = X + (size_t)lr * LDX + 4 * lh;
    const float* xa1 = X + (size_t)(32 + lr) * LDX + 4 * lh;
    const float* wb[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int cb = imax(0, wave + 4 * j < NCB ? wave + 4 * j : 0);
        wb[j] = W + (size_t)(cb * 32 + lr) * ldw + 4 * lh;
    }
    float4 bn[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) bn[j] = *reinterpret_cast<const float4*>(wb[j]);
#pragma unroll 2
    for (int q = 0; q < K / 8; ++q) {
        float4 b[NJ];
#pragma unroll
        for (int j = 0; j < NJ; ++j) b[j] = bn[j];
        if (q + 1 < K / 8) {
#pragma unroll
            for (int j = 0; j < NJ; ++j) bn[j] = *reinterpret_cast<const float4*>(wb[j] + 8 * (q + 1));
        }
        const float4 a0 = *reinterpret_cast<const float4*>(xa0 + 8 * q);
        const float4 a1 = *reinterpret_cast<const float4*>(xa1 + 8 * q);
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            if (wave + 4 * j < NCB) {
                acc[0][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0.x, b[j].x, acc[0][j], 0, 0, 0);
                acc[1][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1.x, b[j].x, acc[1][j], 0, 0, 0);
                acc[0][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0.y, b[j].y, acc[0][j], 0, 0, 0);
                acc[1][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1.y, b[j].y, acc[1][j], 0, 0, 0);
                acc[0][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0.z, b[j].z, acc[0][j], 0, 0, 0);
                acc[1][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1.z, b[j].z, acc[1][j], 0, 0, 0);
                acc[0][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0.w, b[j].w, acc[0][j], 0, 0, 0);
                acc[1][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1.w, b[j].w, acc[1][j], 0, 0, 0);
            }
        }
    }
}

// acc[rb][j] = X[rb*32 + row][k] * W[(w + 4j)*32 + col][k] over k < K (W [*, K] in global memory)
template <int K, int LDX, int NJ, int NCB>
__device__ __forceinline__ void mfma_layer(const float* __restrict__ X, const float* __restrict__ W, int wave, int lane,
                                           f32x16 (&acc)[2][NJ]) {
    acc_clear(acc);
    mfma_layer_acc<K, LDX, NJ, NCB>(X, W, K, wave, lane, acc);
}

// acc[rb][j] += X[rb*32 + row][k] * W[(w + 4j)*32 + col][k] over k < K, bf16 products accumulated in fp32; acc is NOT cleared.
// X in LDS with row stride LDX elements; W bf16 with row stride ldw elements -- as for mfma_layer_acc the tile may hold columns
// [k0, k0 + K) of a wider input, W then points at column k0 of a [*, ldw] matrix (16-byte aligned there, ldw a multiple of 8).
// Chunks accumulated in ascending order give one fp32 accumulation per element over k-blocks of 16 ascending across the whole
// width.  NRB row blocks of 32 (2: the 64-row tile; 4: a 128-row tile whose weight pieces are loaded once for twice the rows);
// an element's sum is the same chain for every NRB.  UNROLL: k-blocks per trip of the loop (by default all of them: no loop); a
// caller that runs the step inside a loop over column passes on an unchanged tile takes fewer, or the compiler lifts every read
// of the tile out of that loop and into more registers than there are.
template <int K, int LDX, int NJ, int NCB, int NRB = 2, int UNROLL = K / 16>
__device__ __forceinline__ void mfma_layer_bf16_acc(const __bf16* __restrict__ X, const __bf16* __restrict__ W, int ldw, int wave,
                                                    int lane, f32x16 (&acc)[NRB][NJ]) {
    static_assert(K % 16 == 0 && LDX % 8 == 0, "16-byte pieces");
    const int lr = lane & 31, lh = lane >> 5;
    const __bf16* xa[NRB];
#pragma unroll
    for (int rb = 0; rb < NRB; ++rb) xa[rb] = X + (size_t)(rb * 32 + lr) * LDX + 8 * lh;
    const __bf16* wb[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int cb = imax(0, wave + 4 * j < NCB ? wave + 4 * j : 0);
        wb[j] = W + (size_t)(cb * 32 + lr) * ldw + 8 * lh;
    }
    bf16x8 bn[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) bn[j] = *reinterpret_cast<const bf16x8*>(wb[j]);
#pragma unroll UNROLL
    for (int q = 0; q < K / 16; ++q) {
        bf16x8 b[NJ];
#pragma unroll
        for (int j = 0; j < NJ; ++j) b[j] = bn[j];
        if (q + 1 < K / 16) {
#pragma unroll
            for (int j = 0; j < NJ; ++j) bn[j] = *reinterpret_cast<const bf16x8*>(wb[j] + 16 * (q + 1));
        }
        bf16x8 a[NRB];
#pragma unroll
        for (int rb = 0; rb < NRB; ++rb) a[rb] = *reinterpret_cast<const bf16x8*>(xa[rb] + 16 * q);
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            if (wave + 4 * j < NCB) {
#pragma unroll
                for (int rb = 0; rb < NRB; ++rb) acc[rb][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[rb], b[j], acc[rb][j], 0, 0, 0);
            }
        }
    }
}

// acc[rb][j] = X[rb*32 + row][k] * W[(w + 4j)*32 + col][k] over k < K (W [*, K] bf16 in global memory): the step above from zero
template <int K, int LDX, int NJ, int NCB, int NRB = 2, int UNROLL = K / 16>
__device__ __forceinline__ void mfma_layer_bf16(const __bf16* __restrict__ X, const __bf16* __restrict__ W, int wave, int lane,
                                                f32x16 (&acc)[NRB][NJ]) {
    acc_clear(acc);
    mfma_layer_bf16_acc<K, LDX, NJ, NCB, NRB, UNROLL>(X, W, K, wave, lane, acc);
}

// four consecutive channels of one row into a tile: one 16-byte (fp32) or 8-byte (bf16, rounded to nearest even) store
template <typename XT>
__device__ __forceinline__ void tile_store4(XT* p, const float (&z)[4]) {
    if constexpr (std::is_same_v<XT, float>) {
        *reinterpret_cast<float4*>(p) = make_float4(z[0], z[1], z[2], z[3]);
    } else {
        bf16x4 zb;
#pragma unroll
        for (int i = 0; i < 4; ++i) zb[i] = (__bf16)z[i];
        *reinterpret_cast<bf16x4*>(p) = zb;
    }
}

// One layer of a tile, LDS to LDS: Y[row][col] = XT(act(scl[col] * (X W^T) + shf[col])), the epilogue in fp32, on mfma_layer (XT
// float, W fp32) or mfma_layer_bf16 (XT __bf16, W bf16) by the tile's element type.  X has row stride LDX, Y row stride LDY; W is
// [CO][K].  A layer whose epilogue does anything more (a store to global memory, a per-cloud bias, a max) keeps its own loop
// over acc_row.
template <int K, int LDX, int CO, int LDY, int NRB = 2, typename XT>
__device__ __forceinline__ void tile_layer(const XT* X, const void* W, const float* scl, const float* shf, float slope, XT* Y, int wave,
                                           int lane) {
    constexpr int NCB = CO / 32, NJ = (NCB + 3) / 4;
    const int lr = lane & 31, lh = lane >> 5;
    f32x16 acc[NRB][NJ];
    if constexpr (std::is_same_v<XT, float>) mfma_layer<K, LDX, NJ, NCB>(X, static_cast<const float*>(W), wave, lane, acc);
    else mfma_layer_bf16<K, LDX, NJ, NCB, NRB>(X, static_cast<const __bf16*>(W), wave, lane, acc);
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int cb = wave + 4 * j;
        if (cb < NCB) {
            const int col = cb * 32 + lr;
            const float sc = scl[col], sh = shf[col];
            XT* y = Y + col;
#pragma unroll
            for (int rb = 0; rb < NRB; ++rb)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int row = acc_row(rb, r, lh);
                    y[row * LDY] = (XT)act(sc * acc[rb][j][r] + sh, slope);
                }
        }
    }
}

// The last layer under a max, in passes of MAX_PASS columns over [c_begin, c_end): z = scale * (X W^T) + shift (ACT: and the
// activation), rows >= nrows selected to -inf, the max over the lane's 32 rows in registers, then across the two lane halves
// -> part[col]; z reaches neither LDS nor memory.  On mfma_layer (XT float) or mfma_layer_bf16 (XT __bf16) by the tile's element
// type, W [*, K] of that type; the epilogue, the max and part are fp32 either way.  UNROLL: mfma_layer_bf16's k-blocks per trip.
// This is the loop over column passes on an unchanged tile that its comment speaks of: at K = 512 fully unrolled the compiler
// lifted all 64 ds_read_b128 of the tile out of the pass loop (256 registers, 452 B of scratch per lane); that caller takes 8.
template <int K, int LDX, bool ACT, int UNROLL = K / 16, typename XT>
__device__ __forceinline__ void max_passes(const XT* X, const XT* __restrict__ W, const float* __restrict__ scl,
                                           const float* __restrict__ shf, float slope, int nrows, float* __restrict__ part, int c_begin,
                                           int c_end, int wave, int lane) {
    W += (size_t)c_begin * K; scl += c_begin; shf += c_begin; part += c_begin;      // the passes count columns from c_begin
    const int lr = lane & 31, lh = lane >> 5;
    for (int c0 = 0; c0 < c_end - c_begin; c0 += MAX_PASS) {
        f32x16 acc[2][MAX_NJ];
        if constexpr (std::is_same_v<XT, float>) mfma_layer<K, LDX, MAX_NJ, 4 * MAX_NJ>(X, W + (size_t)c0 * K, wave, lane, acc);
        else mfma_layer_bf16<K, LDX, MAX_NJ, 4 * MAX_NJ, 2, UNROLL>(X, W + (size_t)c0 * K, wave, lane, acc);
#pragma unroll
        for (int j = 0; j < MAX_NJ; ++j) {
            const int col = c0 + (wave + 4 * j) * 32 + lr;
            const float sc = scl[col], sh = shf[col];
            float mx = -INFINITY;
#pragma unroll
            for (int rb = 0; rb < 2; ++rb)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const float u = sc * acc[rb][j][r] + sh;
                    const float z = ACT ? act(u, slope) : u;
                    mx = fmaxf(mx, acc_row(rb, r, lh) < nrows ? z : -INFINITY);
                }
            mx = fmaxf(mx, __shfl_xor(mx, 32));
            if (lh == 0) part[col] = mx;
        }
    }
}

// A workgroup's tile of ONE cloud, numbered tile-major (blockIdx.x = t * B + b: the tiles that ragged clouds leave empty are the
// high t of every cloud and are dispatched last): tile t of cloud b, whose nb = clamp(n_valid[b], 1, N) points start at row 0;
// the tile's first row and how many of its rows are points.  An empty tile is one of pad rows only; the caller leaves on it
// ahead of every barrier (the exit is uniform).
struct CloudTile {
    int t, b, nb, row0, nrows;
    __device__ bool empty() const { return row0 >= nb; }
};

template <int ROWS>
__device__ __forceinline__ CloudTile cloud_tile(int B, int N, const int32_t* n_valid) {
    CloudTile c;
    c.t = blockIdx.x / B;
    c.b = blockIdx.x - c.t * B;
    c.nb = n_valid ? min(max(n_valid[c.b], 1), N) : N;
    c.row0 = c.t * ROWS;
    c.nrows = min(ROWS, c.nb - c.row0);
    return c;
}

// The K = 3 layer to 64 channels from a cloud's coordinates xb at the caller's strides (sn per point, sc per coordinate), four
// channels per thread: y = fmaf(w2, z, fmaf(w1, y, w0 * x)), X1[r] = XT(act(scl * y + shf)) for the ROWS rows from row0 (rows
// beyond the capacity N repeat row N - 1).  XFORM: the point first goes through T [3][3], p' = p T, the same chain in ascending k.
// STORE: the rows < nrows also go to Fr (global, row stride ldf, Fr at the tile's first row), in fp32.
template <typename XT, int ROWS, int LDY, bool XFORM, bool STORE>
__device__ __forceinline__ void points_layer(const float* xb, size_t sn, size_t sc, int N, int row0, const float* T, const float* W0,
                                             int ldw0, const float* scl, const float* shf, float slope, XT* X1, float* Fr, int ldf,
                                             int nrows, int tid) {
    constexpr int TPR = 64 / 4;                    // threads per row
    const int c4 = (tid % TPR) * 4;
    float w[4][3], sc1[4], sh1[4], t[9];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
#pragma unroll
        for (int d = 0; d < 3; ++d) w[i][d] = W0[(size_t)(c4 + i) * ldw0 + d];
        sc1[i] = scl[c4 + i]; sh1[i] = shf[c4 + i];
    }
    if (XFORM) {
#pragma unroll
        for (int i = 0; i < 9; ++i) t[i] = T[i];
    }
    for (int r = tid / TPR; r < ROWS; r += NT / TPR) {
        const float* p = xb + (size_t)min(row0 + r, N - 1) * sn;
        float px = p[0], py = p[sc], pz = p[2 * sc];
        if (XFORM) {
            const float qx = fmaf(pz, t[6], fmaf(py, t[3], px * t[0]));
            const float qy = fmaf(pz, t[7], fmaf(py, t[4], px * t[1]));
            const float qz = fmaf(pz, t[8], fmaf(py, t[5], px * t[2]));
            px = qx; py = qy; pz = qz;
        }
        float z[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const float y = fmaf(w[i][2], pz, fmaf(w[i][1], py, w[i][0] * px));
            z[i] = act(sc1[i] * y + sh1[i], slope);
        }
        tile_store4(X1 + r * LDY + c4, z);
        if (STORE && r < nrows) *reinterpret_cast<float4*>(Fr + (size_t)r * ldf + c4) = make_float4(z[0], z[1], z[2], z[3]);
    }
}

// out[b][c] = max over the cloud's ceil(nb / 64) live tiles of part [B * tpc][C], in ascending tile order: the second, small
// launch behind every max over a cloud's points.  grid (B, C / NT).  C is a template argument: with the tile stride a constant the
// loop is compiled with two loads in flight, with a run-time stride with one, which measured about 1 us slower per forward.
template <int C>
__global__ __launch_bounds__(NT) void tile_max_kernel(const float* __restrict__ part, const int32_t* __restrict__ n_valid, int N, int tpc,
                                                      float* __restrict__ out, int ldo) {
    const int b = blockIdx.x, c = blockIdx.y * NT + threadIdx.x;
    const int nb = n_valid ? min(max(n_valid[b], 1), N) : N;
    const int live = (nb + RT - 1) / RT;
    const float* p = part + (size_t)b * tpc * C + c;
    float mx = p[0];
    for (int t = 1; t < live; ++t) mx = fmaxf(mx, p[(size_t)t * C]);
    out[(size_t)b * ldo + c] = mx;
}

}  // namespace infer
}  // namespace pcl
