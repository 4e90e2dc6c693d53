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
// The tile sizes, the MFMA step and the accumulator-to-row map (infer::acc_row) come from infer_mfma.h; fp_layer keeps its own
// epilogue loop (a run-time activation flag, the tap and the ragged zeroing are this kernel's alone).
//
// RAGGED (pcl_fp_level_infer_ragged_f32): cloud b's target rows are its first n = clamp(n_valid[b], 1, N); every wave forms the tile's
// 64-bit row-validity mask with one ballot.  A tile without a valid row stores its zeros and leaves before any layer work; in a mixed
// tile the pad rows ride along (every row of the MFMA products depends on its own row of X only, so whatever a pad row of Us / fs
// holds -- NaN included -- stays in that row) and are stored as exact zeros.  The dense instantiation is the code it was.
#include "common.h"
#include "infer_mfma.h"

namespace pcl {
namespace {

using namespace infer;

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
    const int32_t* n_valid; int tapw;             // ragged only: target rows per cloud [B]; columns of the tapped layer
};

template <int L, int C1, int C2, int C3, int C4, int C5>
struct FpShape {
    static constexpr int LDA = imax(C1, C3) + row_pad<float>;            // X1: layers 1, 3
    static constexpr int LDB = imax(C2, C4) + row_pad<float>;            // X2: layers 2, 4 (L >= 3)
    static constexpr size_t lds_bytes = 4 * (size_t)RT * (LDA + (L >= 3 ? LDB : 0));
};

// layer l >= 1 (0-based): z = act?(scale W_l x + shift) from X (LDS) into Y (LDS), or -- LAST -- into out
template <int l, int K, int LDX, int CO, int LDY, bool LAST, bool RAGGED>
__device__ __forceinline__ void fp_layer(const FpArgs& a, const float* X, float* Y, int wave, int lane, int row0, int nvalid,
                                         unsigned long long vmask) {
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
                    const int row = acc_row(rb, r, lh);
                    float z = sc * acc[rb][j][r] + sh;
                    if (do_act) z = act(z, a.slope);
                    float zs = z;                                          // what is stored: exact zeros on a cloud's pad rows
                    if constexpr (RAGGED) zs = (vmask >> row) & 1 ? z : 0.f;
                    if (LAST) {
                        if (row < nvalid && col < a.ncols) a.out[(size_t)(row0 + row) * a.ldo + col] = zs;
                    } else {
                        Y[(size_t)row * LDY + col] = z;
                        if (tap && row < nvalid) tap[(size_t)(row0 + row) * a.ldt + col] = zs;
                    }
                }
        }
    }
}

template <int L, int C1, int C2, int C3, int C4, int C5, bool RAGGED>
__global__ __launch_bounds__(NT, 2) void fp_level_infer_kernel(const FpArgs a) {
    using S = FpShape<L, C1, C2, C3, C4, C5>;
    constexpr int LDA = S::LDA, LDB = S::LDB;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* X1 = smem;                                        // [RT][LDA]
    float* X2 = X1 + RT * LDA;                               // [RT][LDB] (L >= 3)
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int row0 = blockIdx.x * RT;
    const int nvalid = min(RT, a.R - row0);
    unsigned long long vmask = ~0ull;                        // bit r: tile row r is a point of its cloud (ragged)
    if constexpr (RAGGED) {
        const int gr = row0 + min(lane, nvalid - 1), b = gr / a.N;
        vmask = __ballot(lane < nvalid && gr - b * a.N < min(max(a.n_valid[b], 1), a.N));      // the same in every wave
        if (vmask == 0) {                                    // pad rows only: zeros, no layer work (uniform exit, ahead of every barrier)
            for (int i = tid; i < nvalid * a.ncols; i += NT) a.out[(size_t)(row0 + i / a.ncols) * a.ldo + i % a.ncols] = 0.f;
            if (a.tap_layer >= 0)
                for (int i = tid; i < nvalid * a.tapw; i += NT) a.tap[(size_t)(row0 + i / a.tapw) * a.ldt + i % a.tapw] = 0.f;
            return;
        }
    }

    // 1. layer 1 (the folded first conv): a thread always works on the same four channels (NT is a multiple of C1 / 4)
    static_assert(NT % (C1 / 4) == 0, "layer-1 channel split");
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
        for (int r = tid / (C1 / 4); r < RT; r += NT / (C1 / 4)) {
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
        fp_layer<1, C1, LDA, C2, 0, true, RAGGED>(a, X1, nullptr, wave, lane, row0, nvalid, vmask);
    } else {
        fp_layer<1, C1, LDA, C2, LDB, false, RAGGED>(a, X1, X2, wave, lane, row0, nvalid, vmask);
        __syncthreads();
        if constexpr (L == 3) {
            fp_layer<2, C2, LDB, C3, 0, true, RAGGED>(a, X2, nullptr, wave, lane, row0, nvalid, vmask);
        } else {
            static_assert(L == 5, "FP level kernels: L = 2, 3 or 5");
            fp_layer<2, C2, LDB, C3, LDA, false, RAGGED>(a, X2, X1, wave, lane, row0, nvalid, vmask);
            __syncthreads();
            fp_layer<3, C3, LDA, C4, LDB, false, RAGGED>(a, X1, X2, wave, lane, row0, nvalid, vmask);
            __syncthreads();
            fp_layer<4, C4, LDB, C5, 0, true, RAGGED>(a, X2, nullptr, wave, lane, row0, nvalid, vmask);
        }
    }
}

template <int L, int C1, int C2, int C3, int C4, int C5, bool RAGGED>
int launch_fp(const char* who, const FpArgs& a, hipStream_t st) {
    using S = FpShape<L, C1, C2, C3, C4, C5>;
    constexpr size_t lds = S::lds_bytes;
    static_assert(lds <= 80 * 1024, "two workgroups per CU");
    auto kern = fp_level_infer_kernel<L, C1, C2, C3, C4, C5, RAGGED>;
    if (int rc = lds_opt_in(kern, lds, who)) return rc;
    const int blocks = (a.R + RT - 1) / RT;
    hipLaunchKernelGGL(kern, dim3(blocks), dim3(NT), lds, st, a);
    return check_launch(who);
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

template <bool RAGGED>
static int fp_run(const char* who, const float* Us, const float* skip_small, const float* Ws_small, int CS, int ldw, const float* Uc,
                  const int32_t* idx3, const float* w3, int S, const float* cloud_bias, const int32_t* n_valid, int B, int N, int L,
                  const int32_t* widths, const float* const* W, const float* const* scale, const float* const* shift,
                  int act_mask, float slope, float* out, int ldo, float* tap, int tap_layer, int ldt, void* stream) {
    PCL_REQUIRE(widths && W && scale && shift, "%s: null host array", who);
    PCL_REQUIRE(!RAGGED || n_valid, "%s: null pointer (n_valid)", who);
    PCL_REQUIRE(L >= 1 && L <= FP_MAXL, "%s: L=%d", who, L);
    int w[FP_MAXL] = {0, 0, 0, 0, 0};
    for (int l = 0; l < L; ++l) w[l] = widths[l];
    const int sid = fp_shape_id(L, w);
    PCL_REQUIRE(sid >= 0, "%s: no kernel for L=%d widths %d/%d/%d/%d/%d (pcl_fp_level_infer_supported)", who, L, w[0], w[1],
                w[2], w[3], w[4]);
    PCL_REQUIRE(out, "%s: null pointer (out)", who);
    PCL_REQUIRE(Us || CS > 0 || Uc || cloud_bias, "%s: layer 1 has no input (Us, skip_small, Uc or cloud_bias)", who);
    PCL_REQUIRE(CS >= 0 && CS <= FP_MAXCS && (CS == 0 || (skip_small && Ws_small && ldw >= CS)),
                "%s: CS=%d inline skip channels (<= %d, with skip_small, Ws_small and ldw >= CS)", who, CS, FP_MAXCS);
    PCL_REQUIRE(!Uc || (idx3 && w3 && S >= 1), "%s: Uc needs idx3, w3 and S >= 1 (null pointer)", who);
    PCL_REQUIRE(B >= 1 && N >= 1, "%s: bad sizes B=%d N=%d", who, B, N);
    PCL_REQUIRE((size_t)B * N < (1u << 31) && (!Uc || (size_t)B * S < (1u << 31)), "%s: too many points", who);
    for (int l = 0; l < L; ++l) PCL_REQUIRE(scale[l] && shift[l] && (l == 0 || W[l]), "%s: layer %d: null pointer", who, l);
    const int CL = w[L - 1];
    PCL_REQUIRE(ldo >= CL, "%s: ldo=%d for %d channels", who, ldo, CL);
    PCL_REQUIRE(!tap || (tap_layer >= 1 && tap_layer <= L - 2 && ldt >= w[tap_layer]),
                "%s: tap_layer=%d (an intermediate MFMA layer, 1..L-2) ldt=%d", who, tap_layer, ldt);
    bool aligned = al16(Us, Uc, cloud_bias);
    for (int l = 1; l < L; ++l) aligned = aligned && al16(W[l]);
    PCL_REQUIRE(aligned, "%s: Us, Uc, cloud_bias and the weights must be 16-byte aligned", who);
    FpArgs a = {};
    a.Us = Us; a.fs = skip_small; a.Wfs = Ws_small; a.CS = CS; a.ldw = ldw;
    a.Uc = Uc; a.idx3 = idx3; a.w3 = w3; a.S = S; a.cb = cloud_bias;
    a.R = B * N; a.N = N;
    for (int l = 0; l < L; ++l) { a.W[l] = W[l]; a.sc[l] = scale[l]; a.sh[l] = shift[l]; }
    a.act_mask = act_mask; a.slope = slope;
    a.out = out; a.ldo = ldo; a.ncols = CL;
    a.tap = tap; a.ldt = ldt; a.tap_layer = tap ? tap_layer : -1;
    a.n_valid = n_valid; a.tapw = tap ? w[tap_layer] : 0;
    hipStream_t st = as_stream(stream);
    switch (sid) {
        case 0: return launch_fp<2, 256, 256, 0, 0, 0, RAGGED>(who, a, st);
        case 1: return launch_fp<2, 256, 128, 0, 0, 0, RAGGED>(who, a, st);
        case 2: return launch_fp<3, 128, 128, 128, 0, 0, RAGGED>(who, a, st);
        case 3: return launch_fp<5, 128, 128, 128, 128, 32, RAGGED>(who, a, st);
        default: return launch_fp<5, 128, 128, 128, 128, 64, RAGGED>(who, a, st);
    }
}

extern "C" int pcl_fp_level_infer_f32(const float* Us, const float* skip_small, const float* Ws_small, int CS, int ldw, const float* Uc,
                                      const int32_t* idx3, const float* w3, int S, const float* cloud_bias, int B, int N, int L,
                                      const int32_t* widths, const float* const* W, const float* const* scale, const float* const* shift,
                                      int act_mask, float slope, float* out, int ldo, float* tap, int tap_layer, int ldt, void* stream) {
    return fp_run<false>("pcl_fp_level_infer_f32", Us, skip_small, Ws_small, CS, ldw, Uc, idx3, w3, S, cloud_bias, nullptr, B, N, L, widths, W,
                         scale, shift, act_mask, slope, out, ldo, tap, tap_layer, ldt, stream);
}

extern "C" int pcl_fp_level_infer_ragged_f32(const float* Us, const float* skip_small, const float* Ws_small, int CS, int ldw, const float* Uc,
                                             const int32_t* idx3, const float* w3, int S, const float* cloud_bias, const int32_t* n_valid,
                                             int B, int N, int L, const int32_t* widths, const float* const* W, const float* const* scale,
                                             const float* const* shift, int act_mask, float slope, float* out, int ldo, float* tap,
                                             int tap_layer, int ldt, void* stream) {
    return fp_run<true>("pcl_fp_level_infer_ragged_f32", Us, skip_small, Ws_small, CS, ldw, Uc, idx3, w3, S, cloud_bias, n_valid, B, N, L,
                        widths, W, scale, shift, act_mask, slope, out, ldo, tap, tap_layer, ldt, stream);
}
