// infer_mfma.h -- the fp32-MFMA layer step shared by the frozen-inference kernels (infer.hip, infer_fp.hip, infer_pointnet.hip).
//
// A workgroup of 4 waves holds a 64-row tile of activations in LDS (row stride LDX).  Wave w owns the 32-column blocks
// w, w+4, ... of both 32-row blocks and accumulates them on v_mfma_f32_32x32x2_f32: A from LDS (ds_read_b128), B straight
// from the weight matrix in L2 (one 16-byte load per lane per 4 k-steps).  The k order inside a block of 8 is permuted
// (lane half h holds k = 8q + 4h + i at k-step 4q + i) identically for A and B, so each lane moves 16-byte pieces; the sum
// is the same set of products in a different order.  Accumulator element r of lane (lr, lh) is row
// rb*32 + (r & 3) + 8*(r >> 2) + 4*lh, column cb*32 + lr.
//
// mfma_layer_bf16 is the same step with bf16 operands (v_mfma_f32_32x32x16_bf16, fp32 accumulation): the tile and the weight
// matrix hold bf16, lane (lr, lh) takes A[row lr][k = 16q + 8lh + j] and W[col lr][k = 16q + 8lh + j], j < 8, as one 16-byte
// piece each at k-block q; the k-blocks run in ascending order and no k permutation is needed.  Same ownership, same
// accumulator map.  LDX = K + 8: rows of (2K + 16) bytes, an odd number of 16-byte pieces, so the 16-byte reads of
// consecutive rows fall on distinct banks, and every row stays 16-byte aligned.
#pragma once
#include "common.h"

namespace pcl {
namespace infer {

typedef float f32x16 __attribute__((ext_vector_type(16)));

__host__ __device__ constexpr int imax(int a, int b) { return a > b ? a : b; }

__device__ __forceinline__ float act(float u, float slope) { return u > 0.f ? u : u * slope; }

// acc[rb][j] += X[rb*32 + row][k] * W[(w + 4j)*32 + col][k] over k < K (X in LDS with row stride LDX, W [*, K] in global memory)
template <int K, int LDX, int NJ, int NCB>
__device__ __forceinline__ void mfma_layer(const float* __restrict__ X, const float* __restrict__ W, int wave, int lane,
                                           f32x16 (&acc)[2][NJ]) {
    const int lr = lane & 31, lh = lane >> 5;
#pragma unroll
    for (int rb = 0; rb < 2; ++rb)
#pragma unroll
        for (int j = 0; j < NJ; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[rb][j][r] = 0.f;
    const float* xa0 = X + (size_t)lr * LDX + 4 * lh;
    const float* xa1 = X + (size_t)(32 + lr) * LDX + 4 * lh;
    const float* wb[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int cb = imax(0, wave + 4 * j < NCB ? wave + 4 * j : 0);
        wb[j] = W + (size_t)(cb * 32 + lr) * K + 4 * lh;
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

// The K-chunked form of mfma_layer: acc is NOT cleared, and W has row stride ldw -- the tile in LDS holds columns [k0, k0 + K)
// of a wider input and W points at column k0 of a [*, ldw] matrix (16-byte aligned there).  Chunks accumulated in ascending
// order give one fp32 chain per element in the k order of mfma_layer over the whole width.
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

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));

// acc[rb][j] += X[rb*32 + row][k] * W[(w + 4j)*32 + col][k] over k < K, bf16 products accumulated in fp32 (X in LDS with row
// stride LDX elements, W [*, K] bf16 in global memory).  NRB row blocks of 32 (2: the 64-row tile; 4: a 128-row tile whose
// weight pieces are loaded once for twice the rows); an element's sum is the same chain for every NRB.
template <int K, int LDX, int NJ, int NCB, int NRB = 2>
__device__ __forceinline__ void mfma_layer_bf16(const __bf16* __restrict__ X, const __bf16* __restrict__ W, int wave, int lane,
                                                f32x16 (&acc)[NRB][NJ]) {
    static_assert(K % 16 == 0 && LDX % 8 == 0, "16-byte pieces");
    const int lr = lane & 31, lh = lane >> 5;
#pragma unroll
    for (int rb = 0; rb < NRB; ++rb)
#pragma unroll
        for (int j = 0; j < NJ; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[rb][j][r] = 0.f;
    const __bf16* xa[NRB];
#pragma unroll
    for (int rb = 0; rb < NRB; ++rb) xa[rb] = X + (size_t)(rb * 32 + lr) * LDX + 8 * lh;
    const __bf16* wb[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int cb = imax(0, wave + 4 * j < NCB ? wave + 4 * j : 0);
        wb[j] = W + (size_t)(cb * 32 + lr) * K + 8 * lh;
    }
    bf16x8 bn[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) bn[j] = *reinterpret_cast<const bf16x8*>(wb[j]);
#pragma unroll
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

}  // namespace infer
}  // namespace pcl
