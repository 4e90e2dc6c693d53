// infer_pointnet_seg.hip -- PointNet part segmentation in evaluation mode (networks/seg/pointnet_partseg.py:28-41 under
// net.eval()) without the [B, N, 4944] concatenation and without out5.  DESIGN.md section 20 has the algebra; in short the head's
// first layer is folded to K = 832 on a row buffer F [B*N, ldf] = out1 | out2 | out3 | out4 plus a per-cloud bias, and the only
// 2048-wide work left is the pass that produces the global max.  Four launches (each max followed by the per-cloud tile reduce):
//   stn    : STN3d's conv stack 3 -> 64 -> 128 -> 1024 and its max over the points                      -> [B, 1024]
//   trunk  : x' = x T3[b], conv1-3 (3 -> 64 -> 128 -> 128) stored into F[., 0:320], then fstn's conv stack
//            128 -> 64 -> 128 -> 1024 on out3 from LDS and its max                                        -> [B, 1024]
//   global : out3 from F times the cloud's own T128, conv4 128 -> 512 stored into F[., 320:832], conv5 512 -> 2048 (scale / shift,
//            no activation) and its max; out5 reaches neither LDS nor memory                             -> [B, 2048]
//   head   : F[., 0:832] in K-chunks, 832 -> 256 (+ per-cloud bias) -> 256 -> 128 -> part_num, stored as [B, part_num, N]
// plus pcl_pointnet_seg_rows_f32 for the B-row tails (the T-Nets' fully connected layers, the per-cloud bias).
//
// Conventions, all of infer_pointnet.hip: a workgroup (4 waves) owns one 64-row tile of ONE cloud, numbered tile-major
// (blockIdx.x = t * B + b); a tile whose first row is >= n_b leaves before any load (the head kernel first stores its zeros);
// rows >= n_b are selected to -inf under a max; per-tile partial maxima go to a never-cleared workspace and are reduced in
// ascending tile order; no atomics, no inter-workgroup hand-off; layers run on infer::mfma_layer.  Rows of a GEMM are
// independent: a pad row inside a live tile (NaN included) stays in that row; rows beyond the capacity repeat row N - 1.
// The pieces both files run live in infer_mfma.h: the tile prologue (infer::cloud_tile), the K = 3 layer (infer::points_layer,
// here also with the 3 x 3 transform and the store into F), the last layer under a max (infer::max_passes) and the tile reduce
// (infer::tile_max_kernel).  seg_layer keeps its own epilogue loop: it alone also stores rows to F and has an identity form.
// There are three kernel bodies, each with one host launcher: seg_front_kernel<TRUNK> (stn and trunk), seg_global_kernel<XT> and
// seg_head_kernel<XT>, XT (float or __bf16) being the element type of the LDS tiles and of the weights.  Row strides and LDS sizes
// follow from row_pad<XT>; seg_stage, seg_layer and infer::max_passes pick their store and their MFMA step by that type.
//
// Numerics: K = 3 layers are fmaf(w2, z, fmaf(w1, y, w0 * x)), the 3 x 3 transform the same chain in ascending k; every other
// layer is one fp32 chain per element in the k order of infer::mfma_layer (the K = 832 layer: its chunks in ascending order, the
// same chain); epilogues are scale * y + shift (two roundings) and the leaky ReLU.  A cloud's results depend only on its own
// valid rows: bit for bit the same for any B, any position in the batch, any capacity N, any pad contents and any run.
//
// XT = __bf16 (pcl_pointnet_seg_global_infer_bf16_f32, pcl_pointnet_seg_head_infer_bf16_f32) puts the wide
// layers on v_mfma_f32_32x32x16_bf16 (infer::mfma_layer_bf16).  stn, trunk, the B-row tails, the tile max, the layout of F (fp32
// [B*N, ldf]) and every scale, shift and bias stay fp32.  Numerics contract:
//   global: out3 is staged from F in fp32; x2 = out3 . T128[b] stays on the fp32 MFMA step (both operands are run-time fp32 data;
//           1.4 % of the launch's FLOPs) with the fp32 kernel's chain; x2 is rounded to nearest even to bf16; conv4 is bf16 x bf16
//           accumulated in fp32, k-blocks of 16 ascending, its epilogue act(scale * y + shift) in fp32; out4 goes to F[., 320:832]
//           in fp32, unrounded, for the rows < n_b, and to the LDS tile rounded to bf16; conv5 is bf16 x bf16 accumulated in fp32,
//           its epilogue scale * y + shift in fp32 with no activation and never rounded; the max, the partials and out are fp32.
//   head:   every staged element of F is rounded to bf16 as it enters LDS (the out4 the head multiplies is the value the global
//           kernel multiplied); layer 1 takes its K-chunks in ascending order: one fp32 accumulation per element over k-blocks of
//           16 ascending across the whole K = 832, then + bias[b] and the epilogue in fp32; z_1, z_2, z_3 are rounded to bf16; all
//           four layers run on bf16 operands, the last one linear + bias_out in fp32; logits are fp32 and never rounded; logits of
//           pad points are exact zeros, also in tiles that do nothing else.
// Weights are bf16, rounded once by the caller (the folded K = 832 weight straight from fp64).  A cloud's results depend only on
// its own valid rows: the same bits for any B, position, capacity N, pad contents (NaN included) and run; no atomics.
#include "common.h"
#include "infer_mfma.h"

namespace pcl {
namespace {

using namespace infer;

// row strides of a tile of XT (float or __bf16): 128 wide (x2, the head's K-chunks; LD128 for float), the 512-wide out4 tile, the
// head's 256-wide tile, and the fp32 view of LDS the head's logits go through (float: the tile itself; __bf16: [RT][LD128])
template <typename XT> constexpr int SG_LD128 = 128 + row_pad<XT>;
template <typename XT> constexpr int SG_LD4 = 512 + row_pad<XT>;
template <typename XT> constexpr int SG_LDH = 256 + row_pad<XT>;
template <typename XT> constexpr int SG_LDO = std::is_same_v<XT, float> ? SG_LDH<float> : LD128;
constexpr int SG_C1 = 64, SG_C2 = 128, SG_C3 = 128, SG_C4 = 512, SG_C5 = 2048, SG_CT = 1024;
constexpr int SG_F2 = SG_C1, SG_F3 = SG_F2 + SG_C2, SG_F4 = SG_F3 + SG_C3, SG_FK = SG_F4 + SG_C4;      // F's column blocks; 832
constexpr int SG_H1 = 256, SG_H2 = 256, SG_H3 = 128, SG_PMAX = 128;
constexpr int SG_CHUNK = 128;      // K-chunk of the head's first layer: 832 = 6 * 128 + 64
constexpr size_t SG_LDS_FRONT = 4 * (size_t)2 * RT * LD128;              // 67 584 B: two workgroups per CU
// the out4 tile: 132 096 B (float, one workgroup per CU) or 66 560 B (__bf16, two)
template <typename XT> constexpr size_t SG_LDS_GLOBAL = sizeof(XT) * RT * SG_LD4<XT>;
template <typename XT> constexpr int SG_WGS_GLOBAL = std::is_same_v<XT, float> ? 1 : 2;
// the head's two chunk buffers, its tile and its logits over them: 67 584 B (float) or 34 816 B (__bf16)
template <typename XT> constexpr size_t SG_LDS_HEAD = sizeof(XT) * 2 * RT * SG_LD128<XT>;
template <typename XT> constexpr bool sg_head_fits = sizeof(XT) * RT * SG_LDH<XT> <= SG_LDS_HEAD<XT> && 4 * RT * SG_LDO<XT> <= SG_LDS_HEAD<XT>;
template <typename XT> constexpr bool sg_global_fits = 4 * RT * LD128 + sizeof(XT) * RT * SG_LD128<XT> <= SG_LDS_GLOBAL<XT>;
static_assert(SG_LD128<float> == LD128, "out3 is staged in fp32 under both precisions");
static_assert(sg_head_fits<float> && sg_head_fits<__bf16>, "the head's tile and its fp32 logits lie over its chunk buffers");
static_assert(sg_global_fits<float> && sg_global_fits<__bf16>, "fp32 out3 and its transform x2 lie inside the out4 tile");
static_assert(SG_CT % MAX_PASS == 0 && SG_C5 % MAX_PASS == 0, "whole passes under the max");

// acc += X W^T on the MFMA step of the tile's element type: X [RT][LDX] in LDS, W fp32 (XT float) or bf16 (XT __bf16) with row
// stride ldw, as infer::mfma_layer_acc / mfma_layer_bf16_acc
template <int K, int LDX, int NJ, int NCB, typename XT>
__device__ __forceinline__ void seg_mma(const XT* X, const void* W, int ldw, int wave, int lane, f32x16 (&acc)[2][NJ]) {
    if constexpr (std::is_same_v<XT, float>) mfma_layer_acc<K, LDX, NJ, NCB>(X, static_cast<const float*>(W), ldw, wave, lane, acc);
    else mfma_layer_bf16_acc<K, LDX, NJ, NCB>(X, static_cast<const __bf16*>(W), ldw, wave, lane, acc);
}

// One layer of a 64-row tile: z = act(scale * (X W^T) + shift) in fp32, or z = X W^T (IDENT: no scale, shift or activation), from
// X (LDS, row stride LDX; W of X's element type) into Y (LDS, row stride LDY) as YT(z) and, when G is not null, its rows < nrows
// into G (global, row stride ldg) unrounded as well.  INPLACE: Y may lie over X -- every wave has finished reading X before any
// writes Y.
template <int K, int LDX, int CO, int LDY, bool INPLACE, bool IDENT = false, typename XT, typename YT>
__device__ __forceinline__ void seg_layer(const XT* X, const void* W, const float* __restrict__ scl, const float* __restrict__ shf,
                                          float slope, YT* Y, float* __restrict__ G, int ldg, int nrows, int wave, int lane) {
    constexpr int NCB = CO / 32, NJ = (NCB + 3) / 4;
    const int lr = lane & 31, lh = lane >> 5;
    f32x16 acc[2][NJ];
    acc_clear(acc);
    seg_mma<K, LDX, NJ, NCB>(X, W, K, wave, lane, acc);
    if (INPLACE) __syncthreads();
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int cb = wave + 4 * j;
        if (cb < NCB) {
            const int col = cb * 32 + lr;
            const float sc = IDENT ? 1.f : scl[col], sh = IDENT ? 0.f : shf[col];
#pragma unroll
            for (int rb = 0; rb < 2; ++rb)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int row = acc_row(rb, r, lh);
                    const float z = IDENT ? acc[rb][j][r] : act(sc * acc[rb][j][r] + sh, slope);
                    Y[row * LDY + col] = (YT)z;
                    if (G && row < nrows) G[(size_t)row * ldg + col] = z;
                }
        }
    }
}

// ------------------------------------------------------------------------------------------------------- stn and trunk
struct SegFrontArgs {
    const float* x; size_t sb, sn, sc;
    const int32_t* n_valid; int B, N, tpc;         // tpc: tiles per cloud = ceil(N / 64)
    const float* T3;                               // TRUNK: [B][3][3], x' = x T3[b]
    const float* W0; int ldw0;                     // the K = 3 layer: STN3d's first conv, or (TRUNK) conv1
    const float* cW[3]; const float* cscl[3]; const float* cshf[3];      // TRUNK: conv1-3 (cW[0] is W0)
    const float* sW[3]; const float* sscl[3]; const float* sshf[3];      // the T-Net's conv stack (STN3d: sW[0] is W0)
    float slope;
    float* F; int ldf;                             // TRUNK: the row buffer
    float* part;                                   // [B * tpc][1024]
};

template <bool TRUNK>
__global__ __launch_bounds__(NT, 2) void seg_front_kernel(const SegFrontArgs a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* X1 = smem;                              // [RT][LD128]
    float* X2 = X1 + RT * LD128;                   // [RT][LD128]
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const CloudTile tile = cloud_tile<RT>(a.B, a.N, a.n_valid);
    if (tile.empty()) return;
    const int b = tile.b, t = tile.t, row0 = tile.row0, nrows = tile.nrows;
    // the K = 3 layer -> X1 (and, TRUNK, on the transformed point and also into F[., 0:64])
    points_layer<float, RT, LD128, TRUNK, TRUNK>(a.x + (size_t)b * a.sb, a.sn, a.sc, a.N, row0, TRUNK ? a.T3 + (size_t)b * 9 : nullptr, a.W0,
                                                 a.ldw0, TRUNK ? a.cscl[0] : a.sscl[0], TRUNK ? a.cshf[0] : a.sshf[0], a.slope, X1,
                                                 TRUNK ? a.F + ((size_t)b * a.N + row0) * a.ldf : nullptr, a.ldf, nrows, tid);
    __syncthreads();
    float *Xa = X1, *Xb = X2;                      // the T-Net's 64-wide first activation, and the other tile
    if (TRUNK) {
        float* Fr = a.F + ((size_t)b * a.N + row0) * a.ldf;
        seg_layer<SG_C1, LD128, SG_C2, LD128, false>(X1, a.cW[1], a.cscl[1], a.cshf[1], a.slope, X2, Fr + SG_F2, a.ldf, nrows, wave, lane);
        __syncthreads();
        seg_layer<SG_C2, LD128, SG_C3, LD128, false>(X2, a.cW[2], a.cscl[2], a.cshf[2], a.slope, X1, Fr + SG_F3, a.ldf, nrows, wave, lane);
        __syncthreads();
        seg_layer<SG_C3, LD128, 64, LD128, false>(X1, a.sW[0], a.sscl[0], a.sshf[0], a.slope, X2, nullptr, 0, nrows, wave, lane);
        __syncthreads();
        Xa = X2; Xb = X1;
    }
    seg_layer<64, LD128, 128, LD128, false>(Xa, a.sW[1], a.sscl[1], a.sshf[1], a.slope, Xb, nullptr, 0, nrows, wave, lane);
    __syncthreads();
    max_passes<128, LD128, true>(Xb, a.sW[2], a.sscl[2], a.sshf[2], a.slope, nrows, a.part + ((size_t)b * a.tpc + t) * SG_CT, 0, SG_CT, wave,
                                 lane);
}

// columns [k0, k0 + kw) of the tile's rows of F -> buf [RT][SG_LD128<XT>]: a 16-byte copy (float) or rounded to bf16
template <typename XT>
__device__ __forceinline__ void seg_stage(const float* __restrict__ Fb, int ldf, int N, int row0, int k0, int kw, XT* buf, int tid) {
    const int per = kw / 4;
    for (int i = tid; i < RT * per; i += NT) {
        const int r = i / per, c4 = (i - r * per) * 4;
        const float4 v = *reinterpret_cast<const float4*>(Fb + (size_t)min(row0 + r, N - 1) * ldf + k0 + c4);
        const float z[4] = {v.x, v.y, v.z, v.w};
        tile_store4(buf + r * SG_LD128<XT> + c4, z);
    }
}

// ------------------------------------------------------------------------------------------------------- global
struct SegGlobalArgs {
    float* F; int ldf;
    const int32_t* n_valid; int B, N, tpc;
    const float* TT;                               // [B][128][128]: TT[b][j][k] = T128[b][k][j]
    const float* W[2]; const float* scl[2]; const float* shf[2];       // W[l] point at XT
    float slope;
    float* part;                                   // [B * tpc][2048]
};

template <typename XT>
__global__ __launch_bounds__(NT, SG_WGS_GLOBAL<XT>) void seg_global_kernel(const SegGlobalArgs a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    XT* X4 = reinterpret_cast<XT*>(smem);          // [RT][LD4]: out4; before it exists, out3 and its transform lie inside
    float* X1 = smem;                              // [RT][LD128] fp32: out3
    XT* X2 = reinterpret_cast<XT*>(smem + RT * LD128);      // [RT][SG_LD128<XT>]: x2
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const CloudTile tile = cloud_tile<RT>(a.B, a.N, a.n_valid);
    if (tile.empty()) return;
    const int b = tile.b, t = tile.t, row0 = tile.row0, nrows = tile.nrows;
    const float* Fb = a.F + (size_t)b * a.N * a.ldf;
    seg_stage(Fb, a.ldf, a.N, row0, SG_F3, SG_C3, X1, tid);
    __syncthreads();
    // x2 = out3 . T128[b] on the fp32 step under both precisions, stored as XT
    seg_layer<SG_C3, LD128, SG_C3, SG_LD128<XT>, false, true>(X1, a.TT + (size_t)b * SG_C3 * SG_C3, nullptr, nullptr, a.slope, X2, nullptr, 0,
                                                              nrows, wave, lane);
    __syncthreads();
    float* Fr = a.F + ((size_t)b * a.N + row0) * a.ldf;
    seg_layer<SG_C3, SG_LD128<XT>, SG_C4, SG_LD4<XT>, true>(X2, a.W[0], a.scl[0], a.shf[0], a.slope, X4, Fr + SG_F4, a.ldf, nrows, wave, lane);
    __syncthreads();
    // conv5 under the max: 8 k-blocks per trip of the bf16 step (infer::max_passes on why)
    max_passes<SG_C4, SG_LD4<XT>, false, 8>(X4, reinterpret_cast<const XT*>(a.W[1]), a.scl[1], a.shf[1], a.slope, nrows,
                                            a.part + ((size_t)b * a.tpc + t) * SG_C5, 0, SG_C5, wave, lane);
}

// ------------------------------------------------------------------------------------------------------- head
struct SegHeadArgs {
    const float* F; int ldf;
    const int32_t* n_valid; int B, N, tpc;
    const float* bias; int ldb;                    // [B][256] per-cloud bias of layer 1 (added before its scale / shift)
    const float* W[4]; const float* scl[3]; const float* shf[3];       // W[l] point at XT
    const float* bout; int part_num;
    float slope;
    float* out; size_t ob, oc, on;
};

template <typename XT>
__global__ __launch_bounds__(NT, 2) void seg_head_kernel(const SegHeadArgs a) {
    constexpr int LDC = SG_LD128<XT>, LDH = SG_LDH<XT>, LDO = SG_LDO<XT>;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    XT* S = reinterpret_cast<XT*>(smem);           // the two chunk buffers [RT][LDC]
    XT* Y = S;                                     // [RT][LDH], over them once layer 1 has read them
    float* Yo = smem;                              // [RT][LDO] fp32: the logits on their way to the transposed store
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, lr = lane & 31, lh = lane >> 5;
    const CloudTile tile = cloud_tile<RT>(a.B, a.N, a.n_valid);
    const int b = tile.b, row0 = tile.row0, nrows = tile.nrows;
    float* ob = a.out + (size_t)b * a.ob;
    if (tile.empty()) {                               // a tile of pad rows only: its logits are zeros; nothing is loaded
        if (row0 + lane < a.N)
            for (int c = wave; c < a.part_num; c += 4) ob[(size_t)c * a.oc + (size_t)(row0 + lane) * a.on] = 0.f;
        return;
    }
    const float* Fb = a.F + (size_t)b * a.N * a.ldf;
    const XT* W1 = reinterpret_cast<const XT*>(a.W[0]);
    // layer 1: 832 -> 256 over K-chunks of 128 (the last one 64), the next chunk staged while this one is multiplied
    constexpr int NFULL = SG_FK / SG_CHUNK, REST = SG_FK - NFULL * SG_CHUNK;
    static_assert(REST == 64 && NFULL % 2 == 0, "the chunk schedule below");
    constexpr int NJ = SG_H1 / 32 / 4;
    f32x16 acc[2][NJ];
    acc_clear(acc);
    seg_stage(Fb, a.ldf, a.N, row0, 0, SG_CHUNK, S, tid);
    __syncthreads();
    for (int c = 0; c < NFULL; ++c) {
        const XT* cur = S + (c & 1) * RT * LDC;
        XT* nxt = S + ((c + 1) & 1) * RT * LDC;
        seg_stage(Fb, a.ldf, a.N, row0, (c + 1) * SG_CHUNK, c + 1 < NFULL ? SG_CHUNK : REST, nxt, tid);
        seg_mma<SG_CHUNK, LDC, NJ, SG_H1 / 32>(cur, W1 + c * SG_CHUNK, SG_FK, wave, lane, acc);
        __syncthreads();
    }
    seg_mma<REST, LDC, NJ, SG_H1 / 32>(S, W1 + NFULL * SG_CHUNK, SG_FK, wave, lane, acc);
    __syncthreads();
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int col = (wave + 4 * j) * 32 + lr;
        const float sc = a.scl[0][col], sh = a.shf[0][col], cb = a.bias[(size_t)b * a.ldb + col];
#pragma unroll
        for (int rb = 0; rb < 2; ++rb)
#pragma unroll
            for (int r = 0; r < 16; ++r) Y[acc_row(rb, r, lh) * LDH + col] = (XT)act(sc * (acc[rb][j][r] + cb) + sh, a.slope);
    }
    __syncthreads();
    seg_layer<SG_H1, LDH, SG_H2, LDH, true>(Y, a.W[1], a.scl[1], a.shf[1], a.slope, Y, nullptr, 0, nrows, wave, lane);
    __syncthreads();
    seg_layer<SG_H2, LDH, SG_H3, LDH, true>(Y, a.W[2], a.scl[2], a.shf[2], a.slope, Y, nullptr, 0, nrows, wave, lane);
    __syncthreads();
    // layer 4: linear + bias in fp32 on the column blocks that hold a part; W[3] has whole blocks of rows (the launcher checks)
    const int ncb = (a.part_num + 31) / 32;
    f32x16 lo[2][1];
    if (wave < ncb) {
        acc_clear(lo);
        seg_mma<SG_H3, LDH, 1, 4>(Y, a.W[3], SG_H3, wave, lane, lo);
    }
    __syncthreads();
    if (wave < ncb) {
        const int col = wave * 32 + lr;
        const float bo = col < a.part_num ? a.bout[col] : 0.f;
#pragma unroll
        for (int rb = 0; rb < 2; ++rb)
#pragma unroll
            for (int r = 0; r < 16; ++r) Yo[acc_row(rb, r, lh) * LDO + col] = lo[rb][0][r] + bo;
    }
    __syncthreads();
    // the output's own layout [B, part_num, N]: a wave stores 64 consecutive points of one part; pad points are zeros
    if (row0 + lane < a.N)
        for (int c = wave; c < a.part_num; c += 4)
            ob[(size_t)c * a.oc + (size_t)(row0 + lane) * a.on] = lane < nrows ? Yo[lane * LDO + c] : 0.f;
}

// ------------------------------------------------------------------------------------------------------- B-row tails
// y[r][c] = act(scale[c] * (x[r] . W[c]) + shift[c]) (scale null: 1): one wave per column with its weight row in registers, the
// rows four at a time (a row beyond R repeats row R - 1 and is not stored).  Lane l sums its k = 4 (l + 64 i) + e in ascending (i, e), then the lanes are summed by halving: a value does not
// depend on how many rows the call has.
// NV: 16-byte pieces per lane (K <= 256 NV); the narrow layers take the small instantiations and their occupancy.
constexpr int SG_ROWS_V = 9;                       // the widest: K <= 2304
template <int NV>
__global__ __launch_bounds__(NT) void seg_rows_kernel(const float* __restrict__ x, int ldx, int R, int K, const float* __restrict__ W,
                                                        const float* __restrict__ scl, const float* __restrict__ shf, float slope,
                                                        float* __restrict__ y, int ldy, int C) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int c = blockIdx.x * 4 + wave;
    if (c >= C) return;
    const int nv = K / 4;
    float4 w[NV];
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const int v = lane + 64 * i;
        w[i] = v < nv ? *reinterpret_cast<const float4*>(W + (size_t)c * K + 4 * v) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    const float sc = scl ? scl[c] : 1.f, sh = shf[c];
    constexpr int RU = 4;                          // rows in flight: independent chains, each the chain of its row alone
    for (int r0 = 0; r0 < R; r0 += RU) {
        float s[RU];
#pragma unroll
        for (int u = 0; u < RU; ++u) s[u] = 0.f;
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const int v = lane + 64 * i;
            if (v < nv) {
#pragma unroll
                for (int u = 0; u < RU; ++u) {
                    const float4 x4 = *reinterpret_cast<const float4*>(x + (size_t)min(r0 + u, R - 1) * ldx + 4 * v);
                    s[u] = fmaf(w[i].w, x4.w, fmaf(w[i].z, x4.z, fmaf(w[i].y, x4.y, fmaf(w[i].x, x4.x, s[u]))));
                }
            }
        }
#pragma unroll
        for (int u = 0; u < RU; ++u) {
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) s[u] += __shfl_xor(s[u], off);
            if (lane == 0 && r0 + u < R) y[(size_t)(r0 + u) * ldy + c] = act(sc * s[u] + sh, slope);
        }
    }
}

bool widths_are(int L, const int32_t* w, int n, const int* want) {
    if (L != n || !w) return false;
    for (int i = 0; i < n; ++i)
        if (w[i] != want[i]) return false;
    return true;
}

bool seg_shape_ok(int stack, int C0, int L, const int32_t* w) {
    static const int stn[] = {SG_C1, 128, SG_CT}, trunk[] = {SG_C1, SG_C2, SG_C3}, fstn[] = {64, 128, SG_CT}, glob[] = {SG_C4, SG_C5},
                     head[] = {SG_H1, SG_H2, SG_H3};
    switch (stack) {
    case PCL_SEG_STN: return C0 == 3 && widths_are(L, w, 3, stn);
    case PCL_SEG_TRUNK: return C0 == 3 && widths_are(L, w, 3, trunk);
    case PCL_SEG_FSTN: return C0 == SG_C3 && widths_are(L, w, 3, fstn);
    case PCL_SEG_GLOBAL: return C0 == SG_C3 && widths_are(L, w, 2, glob);
    case PCL_SEG_HEAD: return C0 == SG_FK && L == 4 && widths_are(3, w, 3, head) && w[3] >= 1 && w[3] <= SG_PMAX;
    }
    return false;
}

int tiles_of(int N) { return (N + RT - 1) / RT; }

// what every launcher asks of its sizes
int seg_sizes_ok(const char* who, int B, int N) {
    PCL_REQUIRE(B >= 1 && N >= 1, "%s: bad sizes B=%d N=%d", who, B, N);
    PCL_REQUIRE((size_t)B * tiles_of(N) < (1u << 31) / RT, "%s: too many points", who);
    return PCL_OK;
}

int seg_rows_ok(const char* who, const float* F, int ldf, size_t f_bytes, int B, int N) {
    PCL_REQUIRE(F, "%s: null pointer (F)", who);
    PCL_REQUIRE(ldf >= SG_FK && ldf % 4 == 0 && al16(F), "%s: F must be 16-byte aligned with a row stride >= %d that is a multiple of 4 (ldf=%d)",
                who, SG_FK, ldf);
    const size_t need = pcl_pointnet_seg_rows_workspace_bytes(B, N, ldf);
    if (f_bytes < need) return fail(PCL_EWS, "%s: row workspace %zu < %zu", who, f_bytes, need);
    return PCL_OK;
}

int seg_part_ok(const char* who, const void* ws, size_t ws_bytes, int B, int N, int C) {
    const size_t need = pcl_pointnet_seg_part_workspace_bytes(B, N, C);
    if (!ws || ws_bytes < need) return fail(PCL_EWS, "%s: workspace %zu < %zu", who, ws_bytes, need);
    PCL_REQUIRE(al16(ws), "%s: the workspace must be 16-byte aligned", who);
    return PCL_OK;
}

}  // namespace
}  // namespace pcl
using namespace pcl;

extern "C" int pcl_pointnet_seg_infer_supported(int stack, int C0, int L, const int32_t* widths) { return seg_shape_ok(stack, C0, L, widths); }

extern "C" size_t pcl_pointnet_seg_part_workspace_bytes(int B, int N, int C) {
    if (B < 1 || N < 1 || C < 1) return 0;
    return 4 * (size_t)B * tiles_of(N) * C;
}

extern "C" size_t pcl_pointnet_seg_rows_workspace_bytes(int B, int N, int ldf) {
    if (B < 1 || N < 1 || ldf < SG_FK) return 0;
    return 4 * (size_t)B * N * ldf;
}

namespace {

// One launcher body per kernel body; every check runs before any HIP call.
// stn (TRUNK false: one stack, the T-Net's, whose first layer is the K = 3 layer) and trunk (conv1-3, then fstn's stack *_s on
// out3; T3, F and the second stack are read and checked only when TRUNK)
template <bool TRUNK>
int seg_front_infer(const char* who, const float* x, size_t stride_b, size_t stride_n, size_t stride_c, const int32_t* n_valid, int B, int N,
                    const float* T3, int L, const int32_t* widths, const float* W0, int ldw0, const float* const* W,
                    const float* const* scale, const float* const* shift, int Ls, const int32_t* widths_s, const float* const* Ws,
                    const float* const* scale_s, const float* const* shift_s, float slope, float* F, int ldf, size_t f_bytes,
                    void* workspace, size_t workspace_bytes, float* out, int ldo, void* stream) {
    PCL_REQUIRE(widths && W && scale && shift && (!TRUNK || (widths_s && Ws && scale_s && shift_s)), "%s: null host array", who);
    PCL_REQUIRE(seg_shape_ok(TRUNK ? PCL_SEG_TRUNK : PCL_SEG_STN, 3, L, widths) && (!TRUNK || seg_shape_ok(PCL_SEG_FSTN, SG_C3, Ls, widths_s)),
                "%s: no kernel for these widths (pcl_pointnet_seg_infer_supported)", who);
    PCL_REQUIRE(x && (!TRUNK || T3) && W0 && out, "%s: null pointer (%s or out)", who, TRUNK ? "x, T3, W0" : "x, W0");
    if (int rc = seg_sizes_ok(who, B, N)) return rc;
    PCL_REQUIRE(ldw0 >= 3 && ldo >= SG_CT, "%s: ldw0=%d ldo=%d", who, ldw0, ldo);
    for (int l = 0; l < 3; ++l)
        PCL_REQUIRE(scale[l] && shift[l] && (l == 0 || W[l]) && (!TRUNK || (scale_s[l] && shift_s[l] && Ws[l])), "%s: layer %d: null pointer",
                    who, l);
    if (TRUNK)
        if (int rc = seg_rows_ok(who, F, ldf, f_bytes, B, N)) return rc;
    if (int rc = seg_part_ok(who, workspace, workspace_bytes, B, N, SG_CT)) return rc;
    bool aligned = al16(W[1], W[2]);
    if (TRUNK) aligned = aligned && al16(Ws[0], Ws[1], Ws[2]);
    PCL_REQUIRE(aligned, "%s: the weights of %s must be 16-byte aligned", who, TRUNK ? "the MFMA layers" : "layers 2-3");
    SegFrontArgs a = {};
    a.x = x; a.sb = stride_b; a.sn = stride_n; a.sc = stride_c;
    a.n_valid = n_valid; a.B = B; a.N = N; a.tpc = tiles_of(N);
    a.W0 = W0; a.ldw0 = ldw0;
    for (int l = 0; l < 3; ++l) {
        if (TRUNK) { a.cW[l] = W[l]; a.cscl[l] = scale[l]; a.cshf[l] = shift[l]; }
        a.sW[l] = TRUNK ? Ws[l] : W[l]; a.sscl[l] = TRUNK ? scale_s[l] : scale[l]; a.sshf[l] = TRUNK ? shift_s[l] : shift[l];
    }
    a.slope = slope;
    if (TRUNK) { a.T3 = T3; a.F = F; a.ldf = ldf; }
    a.part = static_cast<float*>(workspace);
    hipStream_t st = as_stream(stream);
    if (int rc = lds_opt_in(seg_front_kernel<TRUNK>, SG_LDS_FRONT, who)) return rc;
    hipLaunchKernelGGL(seg_front_kernel<TRUNK>, dim3(B * a.tpc), dim3(NT), SG_LDS_FRONT, st, a);
    if (int rc = check_launch(who)) return rc;
    hipLaunchKernelGGL(tile_max_kernel<SG_CT>, dim3(B, SG_CT / NT), dim3(NT), 0, st, a.part, n_valid, N, a.tpc, out, ldo);
    return check_launch(who);
}

// global and head at both precisions: W[l] are fp32 (BF16 false) or bf16 (true) [C_l][C_{l-1}]
template <bool BF16>
int seg_global_infer(const char* who, float* F, int ldf, size_t f_bytes, const int32_t* n_valid, int B, int N, const float* TT, int L,
                     const int32_t* widths, const void* const* W, const float* const* scale, const float* const* shift, float slope,
                     void* workspace, size_t workspace_bytes, float* out, int ldo, void* stream) {
    using XT = std::conditional_t<BF16, __bf16, float>;
    PCL_REQUIRE(widths && W && scale && shift, "%s: null host array", who);
    PCL_REQUIRE(seg_shape_ok(PCL_SEG_GLOBAL, SG_C3, L, widths), "%s: no kernel for these widths (pcl_pointnet_seg_infer_supported)", who);
    PCL_REQUIRE(TT && out, "%s: null pointer (TT or out)", who);
    if (int rc = seg_sizes_ok(who, B, N)) return rc;
    PCL_REQUIRE(ldo >= SG_C5, "%s: ldo=%d", who, ldo);
    for (int l = 0; l < 2; ++l) PCL_REQUIRE(scale[l] && shift[l] && W[l], "%s: layer %d: null pointer", who, l);
    if (int rc = seg_rows_ok(who, F, ldf, f_bytes, B, N)) return rc;
    if (int rc = seg_part_ok(who, workspace, workspace_bytes, B, N, SG_C5)) return rc;
    bool aligned = al16(TT);
    for (int l = 0; l < 2; ++l) aligned = aligned && al16(W[l]);
    PCL_REQUIRE(aligned, "%s: TT and the weights must be 16-byte aligned", who);
    SegGlobalArgs a = {};
    a.F = F; a.ldf = ldf;
    a.n_valid = n_valid; a.B = B; a.N = N; a.tpc = tiles_of(N);
    a.TT = TT;
    for (int l = 0; l < 2; ++l) { a.W[l] = static_cast<const float*>(W[l]); a.scl[l] = scale[l]; a.shf[l] = shift[l]; }
    a.slope = slope;
    a.part = static_cast<float*>(workspace);
    hipStream_t st = as_stream(stream);
    if (int rc = lds_opt_in(seg_global_kernel<XT>, SG_LDS_GLOBAL<XT>, who)) return rc;
    hipLaunchKernelGGL(seg_global_kernel<XT>, dim3(B * a.tpc), dim3(NT), SG_LDS_GLOBAL<XT>, st, a);
    if (int rc = check_launch(who)) return rc;
    hipLaunchKernelGGL(tile_max_kernel<SG_C5>, dim3(B, SG_C5 / NT), dim3(NT), 0, st, a.part, n_valid, N, a.tpc, out, ldo);
    return check_launch(who);
}

template <bool BF16>
int seg_head_infer(const char* who, const float* F, int ldf, size_t f_bytes, const int32_t* n_valid, int B, int N, const float* cloud_bias,
                   int ldb, int L, const int32_t* widths, const void* const* W, int w_out_rows, const float* const* scale,
                   const float* const* shift, const float* bias_out, float slope, float* out, size_t stride_b, size_t stride_c,
                   size_t stride_n, void* stream) {
    using XT = std::conditional_t<BF16, __bf16, float>;
    PCL_REQUIRE(widths && W && scale && shift, "%s: null host array", who);
    PCL_REQUIRE(seg_shape_ok(PCL_SEG_HEAD, SG_FK, L, widths), "%s: no kernel for these widths (pcl_pointnet_seg_infer_supported)", who);
    const int part_num = widths[3];
    PCL_REQUIRE(cloud_bias && bias_out && out, "%s: null pointer (cloud_bias, bias_out or out)", who);
    if (int rc = seg_sizes_ok(who, B, N)) return rc;
    PCL_REQUIRE(ldb >= SG_H1, "%s: ldb=%d", who, ldb);
    PCL_REQUIRE(w_out_rows >= (part_num + 31) / 32 * 32, "%s: the last weight needs %d rows (whole 32-row blocks), has %d", who,
                (part_num + 31) / 32 * 32, w_out_rows);
    for (int l = 0; l < 4; ++l) PCL_REQUIRE(W[l] && (l == 3 || (scale[l] && shift[l])), "%s: layer %d: null pointer", who, l);
    if (int rc = seg_rows_ok(who, F, ldf, f_bytes, B, N)) return rc;
    bool aligned = true;
    for (int l = 0; l < 4; ++l) aligned = aligned && al16(W[l]);
    PCL_REQUIRE(aligned, "%s: the weights must be 16-byte aligned", who);
    SegHeadArgs a = {};
    a.F = F; a.ldf = ldf;
    a.n_valid = n_valid; a.B = B; a.N = N; a.tpc = tiles_of(N);
    a.bias = cloud_bias; a.ldb = ldb;
    for (int l = 0; l < 4; ++l) a.W[l] = static_cast<const float*>(W[l]);
    for (int l = 0; l < 3; ++l) { a.scl[l] = scale[l]; a.shf[l] = shift[l]; }
    a.bout = bias_out; a.part_num = part_num;
    a.slope = slope;
    a.out = out; a.ob = stride_b; a.oc = stride_c; a.on = stride_n;
    hipStream_t st = as_stream(stream);
    if (int rc = lds_opt_in(seg_head_kernel<XT>, SG_LDS_HEAD<XT>, who)) return rc;
    hipLaunchKernelGGL(seg_head_kernel<XT>, dim3(B * a.tpc), dim3(NT), SG_LDS_HEAD<XT>, st, a);
    return check_launch(who);
}

}  // namespace

extern "C" int pcl_pointnet_seg_stn_infer_f32(const float* x, size_t stride_b, size_t stride_n, size_t stride_c, const int32_t* n_valid,
                                              int B, int N, int L, const int32_t* widths, const float* W0, int ldw0, const float* const* W,
                                              const float* const* scale, const float* const* shift, float slope, void* workspace,
                                              size_t workspace_bytes, float* out, int ldo, void* stream) {
    return seg_front_infer<false>("pcl_pointnet_seg_stn_infer_f32", x, stride_b, stride_n, stride_c, n_valid, B, N, nullptr, L, widths, W0, ldw0,
                                  W, scale, shift, 0, nullptr, nullptr, nullptr, nullptr, slope, nullptr, 0, 0, workspace, workspace_bytes, out,
                                  ldo, stream);
}

extern "C" int pcl_pointnet_seg_trunk_infer_f32(const float* x, size_t stride_b, size_t stride_n, size_t stride_c, const int32_t* n_valid,
                                                int B, int N, const float* T3, int L, const int32_t* widths, const float* W0, int ldw0,
                                                const float* const* W, const float* const* scale, const float* const* shift, int Ls,
                                                const int32_t* widths_s, const float* const* Ws, const float* const* scale_s,
                                                const float* const* shift_s, float slope, float* F, int ldf, size_t f_bytes,
                                                void* workspace, size_t workspace_bytes, float* out, int ldo, void* stream) {
    return seg_front_infer<true>("pcl_pointnet_seg_trunk_infer_f32", x, stride_b, stride_n, stride_c, n_valid, B, N, T3, L, widths, W0, ldw0, W,
                                 scale, shift, Ls, widths_s, Ws, scale_s, shift_s, slope, F, ldf, f_bytes, workspace, workspace_bytes, out, ldo,
                                 stream);
}

extern "C" int pcl_pointnet_seg_global_infer_f32(float* F, int ldf, size_t f_bytes, const int32_t* n_valid, int B, int N, const float* TT,
                                                 int L, const int32_t* widths, const float* const* W, const float* const* scale,
                                                 const float* const* shift, float slope, void* workspace, size_t workspace_bytes,
                                                 float* out, int ldo, void* stream) {
    return seg_global_infer<false>("pcl_pointnet_seg_global_infer_f32", F, ldf, f_bytes, n_valid, B, N, TT, L, widths,
                                   reinterpret_cast<const void* const*>(W), scale, shift, slope, workspace, workspace_bytes, out, ldo, stream);
}

extern "C" int pcl_pointnet_seg_global_infer_bf16_f32(float* F, int ldf, size_t f_bytes, const int32_t* n_valid, int B, int N,
                                                      const float* TT, int L, const int32_t* widths, const void* const* W,
                                                      const float* const* scale, const float* const* shift, float slope, void* workspace,
                                                      size_t workspace_bytes, float* out, int ldo, void* stream) {
    return seg_global_infer<true>("pcl_pointnet_seg_global_infer_bf16_f32", F, ldf, f_bytes, n_valid, B, N, TT, L, widths, W, scale, shift,
                                  slope, workspace, workspace_bytes, out, ldo, stream);
}

extern "C" int pcl_pointnet_seg_head_infer_f32(const float* F, int ldf, size_t f_bytes, const int32_t* n_valid, int B, int N,
                                               const float* cloud_bias, int ldb, int L, const int32_t* widths, const float* const* W,
                                               int w_out_rows, const float* const* scale, const float* const* shift, const float* bias_out,
                                               float slope, float* out, size_t stride_b, size_t stride_c, size_t stride_n, void* stream) {
    return seg_head_infer<false>("pcl_pointnet_seg_head_infer_f32", F, ldf, f_bytes, n_valid, B, N, cloud_bias, ldb, L, widths,
                                 reinterpret_cast<const void* const*>(W), w_out_rows, scale, shift, bias_out, slope, out, stride_b, stride_c,
                                 stride_n, stream);
}

extern "C" int pcl_pointnet_seg_head_infer_bf16_f32(const float* F, int ldf, size_t f_bytes, const int32_t* n_valid, int B, int N,
                                                    const float* cloud_bias, int ldb, int L, const int32_t* widths, const void* const* W,
                                                    int w_out_rows, const float* const* scale, const float* const* shift,
                                                    const float* bias_out, float slope, float* out, size_t stride_b, size_t stride_c,
                                                    size_t stride_n, void* stream) {
    return seg_head_infer<true>("pcl_pointnet_seg_head_infer_bf16_f32", F, ldf, f_bytes, n_valid, B, N, cloud_bias, ldb, L, widths, W,
                                w_out_rows, scale, shift, bias_out, slope, out, stride_b, stride_c, stride_n, stream);
}

extern "C" int pcl_pointnet_seg_rows_f32(const float* x, int ldx, int R, int K, const float* W, int C, const float* scale,
                                         const float* shift, float slope, float* y, int ldy, void* stream) {
    const char* who = "pcl_pointnet_seg_rows_f32";
    PCL_REQUIRE(x && W && shift && y, "%s: null pointer (x, W, shift or y)", who);
    PCL_REQUIRE(R >= 1 && C >= 1 && K >= 4 && K % 4 == 0 && K <= 256 * SG_ROWS_V, "%s: bad sizes R=%d K=%d C=%d (K a multiple of 4, <= %d)", who,
                R, K, C, 256 * SG_ROWS_V);
    PCL_REQUIRE(ldx >= K && ldx % 4 == 0 && ldy >= C && al16(x, W), "%s: x and W must be 16-byte aligned, ldx=%d a multiple of 4, ldy=%d", who,
                ldx, ldy);
    hipStream_t st = as_stream(stream);
    const dim3 grid((C + 3) / 4), block(NT);
    if (K <= 256) hipLaunchKernelGGL(seg_rows_kernel<1>, grid, block, 0, st, x, ldx, R, K, W, scale, shift, slope, y, ldy, C);
    else if (K <= 1024) hipLaunchKernelGGL(seg_rows_kernel<4>, grid, block, 0, st, x, ldx, R, K, W, scale, shift, slope, y, ldy, C);
    else hipLaunchKernelGGL(seg_rows_kernel<SG_ROWS_V>, grid, block, 0, st, x, ldx, R, K, W, scale, shift, slope, y, ldy, C);
    return check_launch(who);
}
