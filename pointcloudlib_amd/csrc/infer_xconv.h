// infer_xconv.h -- the kernel text shared by infer_xconv.hip (the stages of networks/cls/pointcnn.py and the C entry points) and
// infer_xconv_seg.hip (the stages of networks/seg/pointcnn_partseg.py): a translation unit instantiates its own shapes, so that
// adding one leaves the code of the others as it was.
//
// One X-conv stage of PointCNN in evaluation mode, up to and including the depthwise taps, as ONE launch
// (misc/pointcnn.py: PointCNN.forward + XConv.forward_local under net.eval()): per region r = (cloud b, representative p)
//
//     d[k]   = pts[idx[k]] - rep                                    the K local coordinates (the subtraction of pcl_group_f32)
//     h1[k]  = relu(sa * (Wa d[k]) + ta),  h2[k] = relu(sb * (Wb h1[k]) + tb)        the lift, 3 -> C_mid -> C_mid
//     x0     = relu(W0 [d[0] .. d[K-1]])                            x_trans_0 (its BatchNorm is folded into W1 / sh1 by the host)
//     x1     = relu(sc1 * (W1 x0) + sh1),   X = W2 x1 + b2          x_trans_1, x_trans_2: X [K, K]
//     FX     = X . [h2 | relu(fs * feat[idx] + ft)],   D[r, c*dm + j] = bias[c*dm + j] + sum_k wd[c, j, k] FX[k, c]     (pcl_xconv_core_fwd_f32's chains)
//
// The k-NN lists are read as pcl_knn_f32 writes them, [B, K*D, P], rows 0, D, 2D, ...: no slice, permute or copy.  Neither X, the
// lift, the gathered rows nor any [B,P,K,.] tensor reaches memory; D [B*P, C*dm] is the only thing a stage writes.
//
// A workgroup (4 waves) owns a run of consecutive regions and walks them in tiles of 16.  Per tile, in LDS:
//   0. records (one thread per (region, k)): source row b*N + idx (idx clamped to [0, N - 1] so that no load leaves the cloud), d ->
//      PT [16][3K padded to a multiple of 16, pad columns zero];
//   1. h1 on the vector pipe (four channels per thread, constants staged in LDS once) -> H [16 K][C_mid padded to 16];
//      x0 on v_mfma_f32_16x16x4_f32: the tile's 16 regions are the rows of one MFMA row block, wave w owns the 16-column blocks
//      w, w + 4, ... of the K*K outputs -> TA [16][K*K];
//   2. h2 on the same MFMA with (region, k) as rows: wave w owns the row blocks w, w + 4, ... with ALL their column blocks, reads
//      the block's rows of H into its accumulators and then writes h2 over them (no other wave touches those rows);
//      x1: TA -> TB;
//   3. X: TB -> TA;
//   4. FX and the taps with xconv.hip's thread map: a thread owns one channel c (two when C > 256) with its dm x K taps in
//      registers for the whole kernel (in LDS at dm = 16), reads X as 16-byte LDS broadcasts, h2 from H and the gathered feature
//      rows from global memory
//      (coalesced along c; the per-point dense's eval BatchNorm and ReLU are applied here, so what is read is its raw GEMM
//      output; a pass's rows are requested a pass ahead, the first pass's ahead of steps 1 - 3), and stores its dm outputs as 8- or
//      16-byte pieces (dm = 1: one float, consecutive threads consecutive columns).
//      The FX form (DM = 0 in the templates below) has no taps: the thread stores FX[k, c] to out[r, k*C + c], k < K -- every
//      store of a wave is one run of consecutive floats along c.  A frozen evaluator contracts those K*C columns with the taps
//      folded into the pointwise weight (pointcloudlib_amd/inference.py: fold_taps) where dm > K.
// MFMA operands: lane (lr = l & 15, g = l >> 4) holds A[row lr][k] and W[col lr][k] for k = 16q + 4g + i at k-step 4q + i -- the k
// order inside a block of 16 is permuted identically for A and B, so both move as 16-byte pieces (A: ds_read_b128 from a tile
// whose row stride is an odd number of 16-byte pieces; B: the weights from L2, next block's piece in flight).  The weights of the
// X-transform (256 KB at K = 16) are never staged: every wave streams its own column blocks.  Zero pad columns add exact zeros.
//
// Numeric contract (include/pcl_hip.h): a region's result depends only on its own rows (not on B, on the region's place in the
// launch or on how many regions a workgroup owns); no atomics, two calls give identical bits.
#pragma once
#include "common.h"

namespace pcl {
namespace xinfer {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int XI_T = 256;                  // threads per workgroup (4 waves)
constexpr int XI_R = 16;                   // regions per tile: one MFMA row block
constexpr int XI_MAXTILES = 8;             // tiles per workgroup at most

__host__ __device__ constexpr int up16(int v) { return (v + 15) / 16 * 16; }

struct XArgs {
    const float* pts; const float* rep; const float* feat; const float* fs; const float* ft; const int32_t* knn;
    int R, N, P, KD, D, RT;
    const float* Wa; const float* sa; const float* ta; const float* Wb; const float* sb; const float* tb;
    const float* W0; const float* W1; const float* sc1; const float* sh1; const float* W2; const float* b2;
    const float* wd; const float* bias;
    float* out; int ldo;
};

template <int K, int CM, int C2, int DM>
struct XShape {
    static constexpr int KK = K * K, D0P = up16(3 * K), CMP = up16(CM), C = CM + C2, ROWS = XI_R * K;
    static constexpr int LDP = D0P + 4, LDT = KK + 4, LDH = CMP + 4;          // odd numbers of 16-byte pieces
    // the depthwise taps of a channel (dm * K) stay in its thread's registers up to 64 of them; more (dm = 16) live in LDS, a
    // channel's taps and biases in a row of LDW floats (an odd number of 16-byte pieces)
    static constexpr bool TAPS_LDS = DM * K > 64;
    static constexpr int LDW = DM * K + DM + 4;
    // PT, TA, TB, H, the source rows, the packed constants of the lift's first layer, the taps
    static constexpr size_t lds_bytes = 4 * ((size_t)XI_R * LDP + 2 * XI_R * LDT + (size_t)ROWS * LDH + ROWS + 5 * CM + (TAPS_LDS ? C * LDW : 0));
    static_assert(ROWS <= XI_T && CM % 4 == 0 && KK % 16 == 0 && K % 4 == 0 && (5 * CM) % 4 == 0 && lds_bytes <= 160 * 1024, "tile");
};

// acc[j] = sum over k < DEPTH of A[lr][k] * W[(cb0 + j*cbs)*16 + lr][k] for the column blocks below ncb (wave-uniform); A in LDS
// with row stride lda, W [*, DEPTH] in global memory, DEPTH a multiple of 16
template <int DEPTH, int NJ>
__device__ __forceinline__ void rows16_gemm(const float* A, int lda, const float* __restrict__ W, int cb0, int cbs, int ncb, int lane,
                                            f32x4 (&acc)[NJ]) {
    static_assert(DEPTH % 16 == 0, "16-byte pieces of a permuted block of 16");
    const int lr = lane & 15, g = lane >> 4;
    const float* pa = A + lr * lda + 4 * g;
    const float* pw[NJ];
    float4 bn[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int cb = cb0 + j * cbs;
        pw[j] = W + (size_t)((cb < ncb ? cb : 0) * 16 + lr) * DEPTH + 4 * g;
        bn[j] = *reinterpret_cast<const float4*>(pw[j]);
        acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
#pragma unroll 2
    for (int q = 0; q < DEPTH / 16; ++q) {
        float4 b[NJ];
#pragma unroll
        for (int j = 0; j < NJ; ++j) b[j] = bn[j];
        if (q + 1 < DEPTH / 16) {
#pragma unroll
            for (int j = 0; j < NJ; ++j) bn[j] = *reinterpret_cast<const float4*>(pw[j] + 16 * (q + 1));
        }
        const float4 a = *reinterpret_cast<const float4*>(pa + 16 * q);
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            if (cb0 + j * cbs < ncb) {
                acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, b[j].x, acc[j], 0, 0, 0);
                acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, b[j].y, acc[j], 0, 0, 0);
                acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, b[j].z, acc[j], 0, 0, 0);
                acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, b[j].w, acc[j], 0, 0, 0);
            }
        }
    }
}

// accumulator element i of lane (lr, g) is row 4g + i, column cb*16 + lr.  MODE 0: relu(acc); 1: relu(sc * acc + sh); 2: acc + sh
template <int MODE>
__device__ __forceinline__ void rows16_store(const f32x4& acc, float* Y, int ldy, int col, const float* __restrict__ sc,
                                             const float* __restrict__ sh, int lane) {
    const int g = lane >> 4;
    const float s = MODE == 1 ? sc[col] : 1.f, t = MODE == 0 ? 0.f : sh[col];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        float v = acc[i];
        if (MODE == 1) v = s * v + t;
        if (MODE == 2) v = v + t;
        if (MODE != 2) v = fmaxf(v, 0.f);
        Y[(4 * g + i) * ldy + col] = v;
    }
}

// one layer of the X-transform on the tile's 16 rows: wave w owns the column blocks w, w + 4, ...
template <int DEPTH, int KK, int MODE>
__device__ __forceinline__ void xtrans_layer(const float* A, int lda, const float* __restrict__ W, const float* __restrict__ sc,
                                             const float* __restrict__ sh, float* Y, int ldy, int wave, int lane) {
    constexpr int NCB = KK / 16, NJ = (NCB + 3) / 4;
    f32x4 acc[NJ];
    rows16_gemm<DEPTH, NJ>(A, lda, W, wave, 4, NCB, lane, acc);
#pragma unroll
    for (int j = 0; j < NJ; ++j)
        if (wave + 4 * j < NCB) rows16_store<MODE>(acc[j], Y, ldy, (wave + 4 * j) * 16 + (lane & 15), sc, sh, lane);
}

template <int K, int CM, int C2, int DM>
__global__ __launch_bounds__(XI_T) void xconv_level_infer_kernel(const XArgs a) {
    using S = XShape<K, CM, C2, DM>;
    constexpr int KK = S::KK, D0P = S::D0P, CMP = S::CMP, C = S::C, ROWS = S::ROWS, LDP = S::LDP, LDT = S::LDT, LDH = S::LDH;
    constexpr bool WIDE = C > XI_T;
    constexpr int NCH = WIDE ? 2 : 1;
    constexpr int SLOTS = WIDE ? 1 : (XI_T / C < XI_R ? XI_T / C : XI_R);
    static_assert(C <= 2 * XI_T, "two channels per thread at most");
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* PT = smem;                                   // [16][LDP]
    float* TA = PT + XI_R * LDP;                        // [16][LDT]
    float* TB = TA + XI_R * LDT;                        // [16][LDT]
    float* H = TB + XI_R * LDT;                         // [16 K][LDH]
    int* srcs = reinterpret_cast<int*>(H + ROWS * LDH); // [16 K]
    float* la = reinterpret_cast<float*>(srcs + ROWS);  // [CM][5]: Wa row, sa, ta

    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int g0 = blockIdx.x * a.RT;
    const int gend = min(g0 + a.RT, a.R);

    // once per workgroup: zero PT and H (their pad columns are never written again), the lift's first-layer constants
    for (int e = tid; e < XI_R * LDP; e += XI_T) PT[e] = 0.f;
    if constexpr (CMP != CM) {
        for (int e = tid; e < ROWS * LDH; e += XI_T) H[e] = 0.f;
    }
    for (int e = tid; e < CM; e += XI_T) {
        la[5 * e] = a.Wa[3 * e]; la[5 * e + 1] = a.Wa[3 * e + 1]; la[5 * e + 2] = a.Wa[3 * e + 2];
        la[5 * e + 3] = a.sa[e]; la[5 * e + 4] = a.ta[e];
    }
    // step 4's thread map (xconv.hip): slot = region of a pass, channel c0 (and c0 + 256); taps and bias in registers -- at dm = 16
    // (128 taps a channel) in LDS instead, rows of LDW floats, so that the kernel keeps several workgroups on a compute unit
    const int slot = WIDE ? 0 : tid / C, c0 = WIDE ? tid : tid % C;
    const bool active = WIDE ? true : slot < SLOTS;
    constexpr bool TAPS_LDS = S::TAPS_LDS;
    constexpr int LDW = S::LDW;
    float* wl = la + 5 * CM;                                      // [C][LDW]: dm x K taps, dm biases (TAPS_LDS)
    constexpr bool FX = DM == 0;                                  // the FX form: no taps, FX itself is the output
    constexpr int DMA = FX ? 1 : DM;
    float w[TAPS_LDS ? 1 : NCH][TAPS_LDS ? 1 : DMA][K], bs[TAPS_LDS ? 1 : NCH][DMA];
    float fsc[NCH], fsh[NCH];                                     // (the eval BatchNorm of the per-point dense, applied on the gather)
#pragma unroll
    for (int h = 0; h < NCH; ++h) {
        const int c = c0 + XI_T * h;
        fsc[h] = (active && c >= CM && c < C) ? a.fs[c - CM] : 0.f;
        fsh[h] = (active && c >= CM && c < C) ? a.ft[c - CM] : 0.f;
        if constexpr (!TAPS_LDS) {
#pragma unroll
            for (int j = 0; j < DM; ++j) {
                bs[h][j] = (active && c < C) ? a.bias[c * DM + j] : 0.f;
#pragma unroll
                for (int k = 0; k < K; ++k) w[h][j][k] = (active && c < C) ? a.wd[(c * DM + j) * K + k] : 0.f;
            }
        }
    }
    if constexpr (TAPS_LDS) {
        for (int e = tid; e < C * DM * K; e += XI_T) wl[(e / (DM * K)) * LDW + e % (DM * K)] = a.wd[e];
        for (int e = tid; e < C * DM; e += XI_T) wl[(e / DM) * LDW + DM * K + e % DM] = a.bias[e];
    }
    // the gathered rows of a pass (raw; channels >= CM only): requested a pass ahead, the first pass's ahead of the tile's layers
    float fcur[NCH][K] = {}, fnext[NCH][K] = {};
    auto request = [&](int s0, int nvalid, float (&f)[NCH][K]) {
        const int rl = s0 + slot;
        if (!active || rl >= nvalid) return;
#pragma unroll
        for (int h = 0; h < NCH; ++h) {
            const int c = c0 + XI_T * h;
            if (c >= CM && c < C) {
#pragma unroll
                for (int k = 0; k < K; ++k) f[h][k] = a.feat[(size_t)srcs[rl * K + k] * C2 + (c - CM)];
            }
        }
    };
    __syncthreads();

    for (int t0 = g0; t0 < gend; t0 += XI_R) {
        const int nvalid = min(XI_R, gend - t0);
        // 0. records; a tile's regions beyond the workgroup's last repeat it (their results are never stored)
        if (tid < ROWS) {
            const int rl = tid / K, k = tid - rl * K;
            const int r = t0 + min(rl, nvalid - 1);
            const int b = r / a.P, p = r - b * a.P;
            const int i = min(max(a.knn[((size_t)b * a.KD + (size_t)k * a.D) * a.P + p], 0), a.N - 1);
            const int src = b * a.N + i;
            const float* pk = a.pts + (size_t)src * 3;
            const float* q = a.rep + (size_t)r * 3;
            float* d = PT + rl * LDP + 3 * k;
            d[0] = __fsub_rn(pk[0], q[0]); d[1] = __fsub_rn(pk[1], q[1]); d[2] = __fsub_rn(pk[2], q[2]);
            srcs[tid] = src;
        }
        __syncthreads();
        request(0, nvalid, fcur);
        // 1. the lift's first layer (vector pipe); x_trans_0 -> TA
        for (int e = tid; e < ROWS * (CM / 4); e += XI_T) {
            const int row = e / (CM / 4), c4 = (e - row * (CM / 4)) * 4;
            const int rl = row / K, k = row - rl * K;
            const float* d = PT + rl * LDP + 3 * k;
            const float dx = d[0], dy = d[1], dz = d[2];
            float z[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const float* cw = la + 5 * (c4 + i);
                const float y = fmaf(cw[2], dz, fmaf(cw[1], dy, cw[0] * dx));
                z[i] = fmaxf(cw[3] * y + cw[4], 0.f);
            }
            *reinterpret_cast<float4*>(H + row * LDH + c4) = make_float4(z[0], z[1], z[2], z[3]);
        }
        xtrans_layer<D0P, KK, 0>(PT, LDP, a.W0, nullptr, nullptr, TA, LDT, wave, lane);
        __syncthreads();
        // 2. the lift's second layer, in place on the wave's own row blocks; x_trans_1 -> TB
        for (int rb = wave; rb < K; rb += 4) {
            constexpr int NCBL = CMP / 16;
            float* Hb = H + rb * 16 * LDH;
            f32x4 acc[NCBL];
            rows16_gemm<CMP, NCBL>(Hb, LDH, a.Wb, 0, 1, NCBL, lane, acc);
#pragma unroll
            for (int j = 0; j < NCBL; ++j) {
                const int col = j * 16 + (lane & 15);
                if (col < CM) rows16_store<1>(acc[j], Hb, LDH, col, a.sb, a.tb, lane);
            }
        }
        xtrans_layer<KK, KK, 1>(TA, LDT, a.W1, a.sc1, a.sh1, TB, LDT, wave, lane);
        __syncthreads();
        // 3. x_trans_2 -> TA = X [16][K][K]
        xtrans_layer<KK, KK, 2>(TB, LDT, a.W2, nullptr, a.b2, TA, LDT, wave, lane);
        __syncthreads();
        // 4. FX = X [h2 | gathered rows] and the depthwise taps: the fmaf chains of pcl_xconv_core_fwd_f32
        for (int s0 = 0; s0 < XI_R; s0 += SLOTS) {
            if (s0 + SLOTS < XI_R) request(s0 + SLOTS, nvalid, fnext);
            const int rl = s0 + slot;
            if (active && rl < nvalid) {
                const float4* x4 = reinterpret_cast<const float4*>(TA + rl * LDT);
#pragma unroll
                for (int h = 0; h < NCH; ++h) {
                    const int c = c0 + XI_T * h;
                    if (c >= C) continue;
                    float f[K], fx[K];
#pragma unroll
                    for (int k = 0; k < K; ++k) f[k] = c < CM ? H[(rl * K + k) * LDH + c] : fmaxf(fsc[h] * fcur[h][k] + fsh[h], 0.f);
#pragma unroll
                    for (int k = 0; k < K; ++k) {
                        float row[K];
#pragma unroll
                        for (int q = 0; q < K / 4; ++q) {
                            const float4 t = x4[k * (K / 4) + q];
                            row[4 * q] = t.x; row[4 * q + 1] = t.y; row[4 * q + 2] = t.z; row[4 * q + 3] = t.w;
                        }
                        float s = 0.f;
#pragma unroll
                        for (int kk = 0; kk < K; ++kk) s = fmaf(row[kk], f[kk], s);
                        fx[k] = s;
                        __builtin_amdgcn_sched_barrier(0);     // (else all K*K LDS values of X are hoisted into registers)
                    }
                    if constexpr (FX) {
                        float* out = a.out + (size_t)(t0 + rl) * a.ldo + c;
#pragma unroll
                        for (int k = 0; k < K; ++k) out[k * C] = fx[k];
                        continue;
                    }
                    float o[DMA];
                    if constexpr (TAPS_LDS) {
                        const float4* w4 = reinterpret_cast<const float4*>(wl + c * LDW);
#pragma unroll
                        for (int j = 0; j < DM; ++j) {
                            float s = wl[c * LDW + DM * K + j];
#pragma unroll
                            for (int q = 0; q < K / 4; ++q) {
                                const float4 t = w4[j * (K / 4) + q];
                                s = fmaf(t.w, fx[4 * q + 3], fmaf(t.z, fx[4 * q + 2], fmaf(t.y, fx[4 * q + 1], fmaf(t.x, fx[4 * q], s))));
                            }
                            o[j] = s;
                        }
                    } else {
#pragma unroll
                        for (int j = 0; j < DM; ++j) {
                            float s = bs[h][j];
#pragma unroll
                            for (int k = 0; k < K; ++k) s = fmaf(w[h][j][k], fx[k], s);
                            o[j] = s;
                        }
                    }
                    float* out = a.out + (size_t)(t0 + rl) * a.ldo + c * DM;
                    if constexpr (DM % 4 == 0) {
#pragma unroll
                        for (int j = 0; j < DM; j += 4) *reinterpret_cast<float4*>(out + j) = make_float4(o[j], o[j + 1], o[j + 2], o[j + 3]);
                    } else if constexpr (DM == 2) {
                        *reinterpret_cast<float2*>(out) = make_float2(o[0], o[1]);
                    } else {
                        static_assert(DM == 1 || FX, "16-, 8- or 4-byte stores");
                        out[0] = o[0];
                    }
                }
            }
#pragma unroll
            for (int h = 0; h < NCH; ++h)
#pragma unroll
                for (int k = 0; k < K; ++k) fcur[h][k] = fnext[h][k];
        }
        __syncthreads();                                       // (the next tile's records and layers overwrite PT, H, TA)
    }
}

// regions per workgroup: whole tiles, XI_MAXTILES of them, halved while the launch would leave compute units without a workgroup
// (K = 16: the tile's LDS admits one workgroup per compute unit) or with fewer than two (K = 8, 12)
int region_tile(int K, int R);                                   // (infer_xconv.hip)

// the stages of networks/seg/pointcnn_partseg.py that have a kernel (infer_xconv_seg.hip): the index of (K, C_mid, C2, dm), dm = 0
// for the FX form, or -1; and the launch of that index
int seg_shape_id(int K, int CM, int C2, int DM);
int seg_launch(int sid, const char* fn, const XArgs& a, hipStream_t st);

template <int K, int CM, int C2, int DM>
int launch(const char* fn, XArgs a, hipStream_t st) {
    using S = XShape<K, CM, C2, DM>;
    a.RT = region_tile(K, a.R);
    auto kern = xconv_level_infer_kernel<K, CM, C2, DM>;
    if (int rc = lds_opt_in(kern, S::lds_bytes, fn)) return rc;
    const int blocks = (a.R + a.RT - 1) / a.RT;
    hipLaunchKernelGGL(kern, dim3(blocks), dim3(XI_T), S::lds_bytes, st, a);
    return check_launch(fn);
}

}  // namespace xinfer
}  // namespace pcl
