// infer_fp.hip -- one PointNet++ feature-propagation level in evaluation mode as ONE launch (misc/ops.py:54-107 and, fused
// behind the last level, the part-seg head of networks/seg/pointnet2_partseg.py:151-176, under net.eval()).
//
// An FP level is mlp(cat(skip, interp)), interp[r] = sum_k w3[r,k] coarse[idx3[r,k]].  Layer 1 is linear, so it is folded:
//     y1[r] = Us[r] (or Ws_small skip_small[r]) + cloud_bias[b] + sum_k w3[r,k] Uc[b, idx3[r,k]],
// with the per-point table Us = skip W0s^T and the coarse table Uc = coarse W0c^T computed ahead by the stats-free GEMM
// (Uc at the coarse resolution: S rows per cloud).  A one-row coarse level (S = 1) and the one-hot class label are
// per-cloud biases.
//
// A workgroup (4 waves) owns one tile of 64 consecutive rows (points):
//   1. layer 1 elementwise, eval BN + activation, four channels per thread -> X1 (LDS);
//   2. layers 2.. on the fp32 MFMA (infer_mfma.h), ping-ponging between X1 and X2 in LDS; each layer has its own
//      (scale, shift) and activation flag;
//   3. the last layer's tile goes straight from the accumulators to out[rows, ldo] (its first `ncols` columns; the last
//      layer may be padded to a 32-multiple with zero weights).  Optionally one intermediate layer is also stored (tap).
// Nothing but the final tile (and the tap) is written to memory; no atomics, so two calls give identical bits.
#include "common.h"
#include "infer_mfma.h"

namespace pcl {
namespace {

using infer::act;
using infer::f32x16;
using infer::imax;
using infer::mfma_layer;

constexpr int FP_T = 256;        // threads per workgroup (4 waves)
constexpr int FP_RT = 64;        // rows per tile (two 32-row MFMA blocks)
constexpr int FP_MAXL = 5;
constexpr int FP_MAXCS = 8;      // inline skip channels at most (FP1: xyz + normal)

struct FpArgs {
    const float* Us; const float* fs; const float* Wfs; int CS, ldw;
    const float* Uc; const int32_t* idx3; const float* w3; int S;
    const float* cb;
    int R, N;
    const float* W[FP_MAXL]; const float* sc[FP_MAXL]; const float* sh[FP_MAXL];
    int act_mask; float slope;
    float* out; int ldo, ncols;
    float* tap; int ldt, tap_layer;
};

template <int L, int C1, int C2, int C3, int C4, int C5>
struct FpShape {
    static constexpr int LDA = imax(C1, C3) + 4;                       // X1: layers 1, 3; +4 floats: ds_read_b128 rows on distinct banks
    static constexpr int LDB = imax(C2, C4) + 4;                       // X2: layers 2, 4 (L >= 3)
    static constexpr size_t lds_bytes = 4 * (size_t)FP_RT * (LDA + (L >= 3 ? LDB : 0));
};

// layer l >= 1 (0-based): z = act?(scale W_l x + shift) from X (LDS) into Y (LDS), or -- LAST -- into out
template <int l, int K, int LDX, int CO, int LDY, bool LAST>
__device__ __forceinline__ void fp_layer(const FpArgs& a, const float* X, float* Y, int wave, int lane, int row0, int nvalid) {
    constexpr int NCB = CO / 32, NJ = (NCB + 3) / 4;
    const int lr = lane & 31, lh = lane >> 5;
    f32x16 acc[2][NJ];
    mfma_layer<K, LDX, NJ, NCB>(X, a.W[l], wave, lane, acc);
    const bool do_act = (a.act_mask >> l) & 1;
    float* tap = a.tap_layer == l ? a.tap : nullptr;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int cb = wave + 4 * j;
        if (cb < NCB) {
            const int col = cb * 32 + lr;
            const float sc = a.sc[l][col], sh = a.sh[l][col];
#pragma unroll
            for (int rb = 0; rb < 2; ++rb)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int row = rb * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
                    float z = sc * acc[rb][j][r] + sh;
                    if (do_act) z = act(z, a.slope);
                    if (LAST) {
                        if (row < nvalid && col < a.ncols) a.out[(size_t)(row0 + row) * a.ldo + col] = z;
                    } else {
                        Y[(size_t)row * LDY + col] = z;
                        if (tap && row < nvalid) tap[(size_t)(row0 + row) * a.ldt + col] = z;
                    }
                }
        }
    }
}

template <int L, int C1, int C2, int C3, int C4, int C5>
__global__ __launch_bounds__(FP_T, 2) void fp_level_infer_kernel(const FpArgs a) {
    using S = FpShape<L, C1, C2, C3, C4, C5>;
    constexpr int LDA = S::LDA, LDB = S::LDB;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* X1 = smem;                                        // [RT][LDA]
    float* X2 = X1 + FP_RT * LDA;                            // [RT][LDB] (L >= 3)
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int row0 = blockIdx.x * FP_RT;
    const int nvalid = min(FP_RT, a.R - row0);

    // 1. layer 1 (the folded first conv): a thread always works on the same four channels (FP_T is a multiple of C1 / 4)
    static_assert(FP_T % (C1 / 4) == 0, "layer-1 channel split");
    {
        const int c4 = (tid % (C1 / 4)) * 4;
        float wf[4][FP_MAXCS], sc1[4], sh1[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
#pragma unroll
            for (int j = 0; j < FP_MAXCS; ++j) wf[i][j] = j < a.CS ? a.Wfs[(size_t)(c4 + i) * a.ldw + j] : 0.f;
            sc1[i] = a.sc[0][c4 + i]; sh1[i] = a.sh[0][c4 + i];
        }
        const bool act1 = a.act_mask & 1;
        for (int r = tid / (C1 / 4); r < FP_RT; r += FP_T / (C1 / 4)) {
            const int gr = row0 + min(r, nvalid - 1);            // the tile's tail repeats its last row (never stored)
            const int b = gr / a.N;
            float y[4] = {0.f, 0.f, 0.f, 0.f};
            if (a.Uc) {
                const int32_t* ii = a.idx3 + (size_t)gr * 3;
                const float* ww = a.w3 + (size_t)gr * 3;
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    const int s = min(max(ii[k], 0), a.S - 1);
                    const float w = ww[k];
                    const float4 u = *reinterpret_cast<const float4*>(a.Uc + ((size_t)b * a.S + s) * C1 + c4);
                    y[0] = fmaf(w, u.x, y[0]); y[1] = fmaf(w, u.y, y[1]); y[2] = fmaf(w, u.z, y[2]); y[3] = fmaf(w, u.w, y[3]);
                }
            }
            if (a.cb) {
                const float4 v = *reinterpret_cast<const float4*>(a.cb + (size_t)b * C1 + c4);
                y[0] += v.x; y[1] += v.y; y[2] += v.z; y[3] += v.w;
            }
            if (a.Us) {
                const float4 v = *reinterpret_cast<const float4*>(a.Us + (size_t)gr * C1 + c4);
                y[0] += v.x; y[1] += v.y; y[2] += v.z; y[3] += v.w;
            }
            if (a.CS) {
                float f[FP_MAXCS];
#pragma unroll
                for (int j = 0; j < FP_MAXCS; ++j) f[j] = j < a.CS ? a.fs[(size_t)gr * a.CS + j] : 0.f;
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int j = 0; j < FP_MAXCS; ++j) y[i] = fmaf(wf[i][j], f[j], y[i]);
            }
            float z[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                z[i] = sc1[i] * y[i] + sh1[i];
                if (act1) z[i] = act(z[i], a.slope);
            }
            *reinterpret_cast<float4*>(X1 + (size_t)r * LDA + c4) = make_float4(z[0], z[1], z[2], z[3]);
        }
    }
    __syncthreads();
    // 2. layers 2..L on the MFMA; the last one to out
    if constexpr (L == 2) {
        fp_layer<1, C1, LDA, C2, 0, true>(a, X1, nullptr, wave, lane, row0, nvalid);
    } else {
        fp_layer<1, C1, LDA, C2, LDB, false>(a, X1, X2, wave, lane, row0, nvalid);
        __syncthreads();
        if constexpr (L == 3) {
            fp_layer<2, C2, LDB, C3, 0, true>(a, X2, nullptr, wave, lane, row0, nvalid);
        } else {
            static_assert(L == 5, "FP level kernels: L = 2, 3 or 5");
            fp_layer<2, C2, LDB, C3, LDA, false>(a, X2, X1, wave, lane, row0, nvalid);
            __syncthreads();
            fp_layer<3, C3, LDA, C4, LDB, false>(a, X1, X2, wave, lane, row0, nvalid);
            __syncthreads();
            fp_layer<4, C4, LDB, C5, 0, true>(a, X2, nullptr, wave, lane, row0, nvalid);
        }
    }
}

template <int L, int C1, int C2, int C3, int C4, int C5>
int launch_fp(const FpArgs& a, hipStream_t st) {
    using S = FpShape<L, C1, C2, C3, C4, C5>;
    constexpr size_t lds = S::lds_bytes;
    static_assert(lds <= 80 * 1024, "two workgroups per CU");
    auto kern = fp_level_infer_kernel<L, C1, C2, C3, C4, C5>;
    if (lds > 64 * 1024) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return fail(PCL_EHIP, "pcl_fp_level_infer_f32: hipFuncSetAttribute(%zu): %s", lds, hipGetErrorString(e));
    }
    const int blocks = (a.R + FP_RT - 1) / FP_RT;
    hipLaunchKernelGGL(kern, dim3(blocks), dim3(FP_T), lds, st, a);
    return check_launch("pcl_fp_level_infer_f32");
}

// the widths after the fold that have a kernel: the FP levels of networks/seg/pointnet2_partseg.py (SSG and MSG) and FP1 with
// the head fused behind it (its last layer: part_num <= 64 classes, padded to 32 or 64)
int fp_shape_id(int L, const int* w) {
    if (L == 2 && w[0] == 256 && w[1] == 256) return 0;
    if (L == 2 && w[0] == 256 && w[1] == 128) return 1;
    if (L == 3 && w[0] == 128 && w[1] == 128 && w[2] == 128) return 2;
    if (L == 5 && w[0] == 128 && w[1] == 128 && w[2] == 128 && w[3] == 128 && w[4] >= 1 && w[4] <= 64) return w[4] <= 32 ? 3 : 4;
    return -1;
}

}  // namespace
}  // namespace pcl
using namespace pcl;

extern "C" int pcl_fp_level_infer_supported(int L, int C1, int C2, int C3, int C4, int C5) {
    const int w[5] = {C1, C2, C3, C4, C5};
    return L >= 1 && L <= FP_MAXL && fp_shape_id(L, w) >= 0;
}

extern "C" int pcl_fp_level_infer_f32(const float* Us, const float* skip_small, const float* Ws_small, int CS, int ldw, const float* Uc,
                                      const int32_t* idx3, const float* w3, int S, const float* cloud_bias, int B, int N, int L,
                                      const int32_t* widths, const float* const* W, const float* const* scale, const float* const* shift,
                                      int act_mask, float slope, float* out, int ldo, float* tap, int tap_layer, int ldt, void* stream) {
    PCL_REQUIRE(widths && W && scale && shift, "pcl_fp_level_infer_f32: null host array");
    PCL_REQUIRE(L >= 1 && L <= FP_MAXL, "pcl_fp_level_infer_f32: L=%d", L);
    int w[FP_MAXL] = {0, 0, 0, 0, 0};
    for (int l = 0; l < L; ++l) w[l] = widths[l];
    const int sid = fp_shape_id(L, w);
    PCL_REQUIRE(sid >= 0, "pcl_fp_level_infer_f32: no kernel for L=%d widths %d/%d/%d/%d/%d (pcl_fp_level_infer_supported)", L, w[0], w[1],
                w[2], w[3], w[4]);
    PCL_REQUIRE(out, "pcl_fp_level_infer_f32: null pointer (out)");
    PCL_REQUIRE(Us || CS > 0 || Uc || cloud_bias, "pcl_fp_level_infer_f32: layer 1 has no input (Us, skip_small, Uc or cloud_bias)");
    PCL_REQUIRE(CS >= 0 && CS <= FP_MAXCS && (CS == 0 || (skip_small && Ws_small && ldw >= CS)),
                "pcl_fp_level_infer_f32: CS=%d inline skip channels (<= %d, with skip_small, Ws_small and ldw >= CS)", CS, FP_MAXCS);
    PCL_REQUIRE(!Uc || (idx3 && w3 && S >= 1), "pcl_fp_level_infer_f32: Uc needs idx3, w3 and S >= 1 (null pointer)");
    PCL_REQUIRE(B >= 1 && N >= 1, "pcl_fp_level_infer_f32: bad sizes B=%d N=%d", B, N);
    PCL_REQUIRE((size_t)B * N < (1u << 31) && (!Uc || (size_t)B * S < (1u << 31)), "pcl_fp_level_infer_f32: too many points");
    for (int l = 0; l < L; ++l) PCL_REQUIRE(scale[l] && shift[l] && (l == 0 || W[l]), "pcl_fp_level_infer_f32: layer %d: null pointer", l);
    const int CL = w[L - 1];
    PCL_REQUIRE(ldo >= CL, "pcl_fp_level_infer_f32: ldo=%d for %d channels", ldo, CL);
    PCL_REQUIRE(!tap || (tap_layer >= 1 && tap_layer <= L - 2 && ldt >= w[tap_layer]),
                "pcl_fp_level_infer_f32: tap_layer=%d (an intermediate MFMA layer, 1..L-2) ldt=%d", tap_layer, ldt);
    bool al16 = ((reinterpret_cast<uintptr_t>(Us) | reinterpret_cast<uintptr_t>(Uc) | reinterpret_cast<uintptr_t>(cloud_bias)) & 15) == 0;
    for (int l = 1; l < L; ++l) al16 = al16 && (reinterpret_cast<uintptr_t>(W[l]) & 15) == 0;
    PCL_REQUIRE(al16, "pcl_fp_level_infer_f32: Us, Uc, cloud_bias and the weights must be 16-byte aligned");
    FpArgs a = {};
    a.Us = Us; a.fs = skip_small; a.Wfs = Ws_small; a.CS = CS; a.ldw = ldw;
    a.Uc = Uc; a.idx3 = idx3; a.w3 = w3; a.S = S; a.cb = cloud_bias;
    a.R = B * N; a.N = N;
    for (int l = 0; l < L; ++l) { a.W[l] = W[l]; a.sc[l] = scale[l]; a.sh[l] = shift[l]; }
    a.act_mask = act_mask; a.slope = slope;
    a.out = out; a.ldo = ldo; a.ncols = CL;
    a.tap = tap; a.ldt = ldt; a.tap_layer = tap ? tap_layer : -1;
    hipStream_t st = as_stream(stream);
    switch (sid) {
        case 0: return launch_fp<2, 256, 256, 0, 0, 0>(a, st);
        case 1: return launch_fp<2, 256, 128, 0, 0, 0>(a, st);
        case 2: return launch_fp<3, 128, 128, 128, 0, 0>(a, st);
        case 3: return launch_fp<5, 128, 128, 128, 128, 32>(a, st);
        default: return launch_fp<5, 128, 128, 128, 128, 64>(a, st);
    }
}
