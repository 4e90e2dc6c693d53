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
// stn and trunk are two instantiations of one kernel body (seg_front_kernel<TRUNK>).
//
// Numerics: K = 3 layers are fmaf(w2, z, fmaf(w1, y, w0 * x)), the 3 x 3 transform the same chain in ascending k; every other
// layer is one fp32 chain per element in the k order of infer::mfma_layer (the K = 832 layer: its chunks in ascending order, the
// same chain); epilogues are scale * y + shift (two roundings) and the leaky ReLU.  A cloud's results depend only on its own
// valid rows: bit for bit the same for any B, any position in the batch, any capacity N, any pad contents and any run.
#include "common.h"
#include "infer_mfma.h"

namespace pcl {
namespace {

using infer::act;
using infer::f32x16;
using infer::mfma_layer;
using infer::mfma_layer_acc;

constexpr int SG_T = 256;          // threads per workgroup (4 waves)
constexpr int SG_RT = 64;          // rows per tile
constexpr int SG_LD = 132;         // row stride of a 128-wide LDS tile (128 + 4: ds_read_b128 rows on distinct banks)
constexpr int SG_LD4 = 516;        // ... of the 512-wide out4 tile
constexpr int SG_LDH = 260;        // ... of the head's 256-wide tile
constexpr int SG_NJ = 2;           // column blocks per wave and pass under a max (64 accumulator registers)
constexpr int SG_PASS = 4 * SG_NJ * 32;
constexpr int SG_C1 = 64, SG_C2 = 128, SG_C3 = 128, SG_C4 = 512, SG_C5 = 2048, SG_CT = 1024;
constexpr int SG_F2 = SG_C1, SG_F3 = SG_F2 + SG_C2, SG_F4 = SG_F3 + SG_C3, SG_FK = SG_F4 + SG_C4;      // F's column blocks; 832
constexpr int SG_H1 = 256, SG_H2 = 256, SG_H3 = 128, SG_PMAX = 128;
constexpr int SG_CHUNK = 128;      // K-chunk of the head's first layer: 832 = 6 * 128 + 64
constexpr size_t SG_LDS_FRONT = 4 * (size_t)2 * SG_RT * SG_LD;           // 67 584 B: two workgroups per CU
constexpr size_t SG_LDS_GLOBAL = 4 * (size_t)SG_RT * SG_LD4;             // 132 096 B: one workgroup per CU
constexpr size_t SG_LDS_HEAD = SG_LDS_FRONT;                             // the two chunk buffers, then the [64][260] tile over them
static_assert(4 * (size_t)SG_RT * SG_LDH <= SG_LDS_HEAD, "the head's tile lies over its chunk buffers");
static_assert(2 * SG_RT * SG_LD <= SG_RT * SG_LD4, "out3 and its transform lie inside the out4 tile");

__device__ __forceinline__ int acc_row(int rb, int r, int lh) { return rb * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh; }

// One layer of a 64-row tile: z = act(scale * (X W^T) + shift), or z = X W^T when scl is null, from X (LDS, row stride LDX) into
// Y (LDS, row stride LDY) and, when G is not null, its rows < nrows into G (global, row stride ldg) as well.  INPLACE: Y may lie
// over X -- every wave has finished reading X before any writes Y.
template <int K, int LDX, int CO, int LDY, bool INPLACE>
__device__ __forceinline__ void seg_layer(const float* X, const float* __restrict__ W, const float* __restrict__ scl,
                                          const float* __restrict__ shf, float slope, float* Y, float* __restrict__ G, int ldg, int nrows,
                                          int wave, int lane) {
    constexpr int NCB = CO / 32, NJ = (NCB + 3) / 4;
    const int lr = lane & 31, lh = lane >> 5;
    f32x16 acc[2][NJ];
    mfma_layer<K, LDX, NJ, NCB>(X, W, wave, lane, acc);
    if (INPLACE) __syncthreads();
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int cb = wave + 4 * j;
        if (cb < NCB) {
            const int col = cb * 32 + lr;
            const float sc = scl ? scl[col] : 1.f, sh = scl ? shf[col] : 0.f;
#pragma unroll
            for (int rb = 0; rb < 2; ++rb)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int row = acc_row(rb, r, lh);
                    const float z = scl ? act(sc * acc[rb][j][r] + sh, slope) : acc[rb][j][r];
                    Y[row * LDY + col] = z;
                    if (G && row < nrows) G[(size_t)row * ldg + col] = z;
                }
        }
    }
}

// The last layer under a max, in passes of 256 columns: z = scale * (X W^T) + shift (ACT: and the activation), rows >= nrows
// selected to -inf, the max over the lane's 32 rows in registers, then across the two lane halves -> part[col], col < C
template <int K, int LDX, int C, bool ACT>
__device__ __forceinline__ void seg_max_passes(const float* X, const float* __restrict__ W, const float* __restrict__ scl,
                                               const float* __restrict__ shf, float slope, int nrows, float* __restrict__ part, int wave,
                                               int lane) {
    static_assert(C % SG_PASS == 0, "whole passes");
    const int lr = lane & 31, lh = lane >> 5;
    for (int c0 = 0; c0 < C; c0 += SG_PASS) {
        f32x16 acc[2][SG_NJ];
        mfma_layer<K, LDX, SG_NJ, 4 * SG_NJ>(X, W + (size_t)c0 * K, wave, lane, acc);
#pragma unroll
        for (int j = 0; j < SG_NJ; ++j) {
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

// the K = 3 layer from the coordinates at the caller's strides, four channels per thread -> X1 (and, TRUNK, F[., 0:64])
template <bool TRUNK>
__device__ __forceinline__ void seg_points_layer(const SegFrontArgs& a, float* X1, int b, int row0, int nrows, int tid) {
    constexpr int TPR = SG_C1 / 4;                 // threads per row
    const float* scl = TRUNK ? a.cscl[0] : a.sscl[0];
    const float* shf = TRUNK ? a.cshf[0] : a.sshf[0];
    const int c4 = (tid % TPR) * 4;
    float w[4][3], sc1[4], sh1[4], T[9];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
#pragma unroll
        for (int d = 0; d < 3; ++d) w[i][d] = a.W0[(size_t)(c4 + i) * a.ldw0 + d];
        sc1[i] = scl[c4 + i]; sh1[i] = shf[c4 + i];
    }
    if (TRUNK) {
#pragma unroll
        for (int i = 0; i < 9; ++i) T[i] = a.T3[(size_t)b * 9 + i];
    }
    const float* xb = a.x + (size_t)b * a.sb;
    for (int r = tid / TPR; r < SG_RT; r += SG_T / TPR) {
        const float* p = xb + (size_t)min(row0 + r, a.N - 1) * a.sn;
        float px = p[0], py = p[a.sc], pz = p[2 * a.sc];
        if (TRUNK) {
            const float qx = fmaf(pz, T[6], fmaf(py, T[3], px * T[0]));
            const float qy = fmaf(pz, T[7], fmaf(py, T[4], px * T[1]));
            const float qz = fmaf(pz, T[8], fmaf(py, T[5], px * T[2]));
            px = qx; py = qy; pz = qz;
        }
        float z[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const float y = fmaf(w[i][2], pz, fmaf(w[i][1], py, w[i][0] * px));
            z[i] = act(sc1[i] * y + sh1[i], a.slope);
        }
        const float4 z4 = make_float4(z[0], z[1], z[2], z[3]);
        *reinterpret_cast<float4*>(X1 + r * SG_LD + c4) = z4;
        if (TRUNK && r < nrows) *reinterpret_cast<float4*>(a.F + ((size_t)b * a.N + row0 + r) * a.ldf + c4) = z4;
    }
}

template <bool TRUNK>
__global__ __launch_bounds__(SG_T, 2) void seg_front_kernel(const SegFrontArgs a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* X1 = smem;                              // [RT][LD]
    float* X2 = X1 + SG_RT * SG_LD;                // [RT][LD]
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int t = blockIdx.x / a.B, b = blockIdx.x - t * a.B;     // tile-major
    const int nb = a.n_valid ? min(max(a.n_valid[b], 1), a.N) : a.N;
    const int row0 = t * SG_RT;
    if (row0 >= nb) return;                        // a tile of pad rows only (uniform exit, ahead of every barrier)
    const int nrows = min(SG_RT, nb - row0);
    seg_points_layer<TRUNK>(a, X1, b, row0, nrows, tid);
    __syncthreads();
    float *Xa = X1, *Xb = X2;                      // the T-Net's 64-wide first activation, and the other tile
    if (TRUNK) {
        float* Fr = a.F + ((size_t)b * a.N + row0) * a.ldf;
        seg_layer<SG_C1, SG_LD, SG_C2, SG_LD, false>(X1, a.cW[1], a.cscl[1], a.cshf[1], a.slope, X2, Fr + SG_F2, a.ldf, nrows, wave, lane);
        __syncthreads();
        seg_layer<SG_C2, SG_LD, SG_C3, SG_LD, false>(X2, a.cW[2], a.cscl[2], a.cshf[2], a.slope, X1, Fr + SG_F3, a.ldf, nrows, wave, lane);
        __syncthreads();
        seg_layer<SG_C3, SG_LD, 64, SG_LD, false>(X1, a.sW[0], a.sscl[0], a.sshf[0], a.slope, X2, nullptr, 0, nrows, wave, lane);
        __syncthreads();
        Xa = X2; Xb = X1;
    }
    seg_layer<64, SG_LD, 128, SG_LD, false>(Xa, a.sW[1], a.sscl[1], a.sshf[1], a.slope, Xb, nullptr, 0, nrows, wave, lane);
    __syncthreads();
    seg_max_passes<128, SG_LD, SG_CT, true>(Xb, a.sW[2], a.sscl[2], a.sshf[2], a.slope, nrows, a.part + ((size_t)b * a.tpc + t) * SG_CT,
                                            wave, lane);
}

// out[b][c] = max over the cloud's live tiles, ascending (pointnet_tile_max_kernel's scheme for C columns)
__global__ __launch_bounds__(SG_T) void seg_tile_max_kernel(const float* __restrict__ part, const int32_t* __restrict__ n_valid, int N,
                                                            int tpc, int C, float* __restrict__ out, int ldo) {
    const int b = blockIdx.x, c = blockIdx.y * SG_T + threadIdx.x;
    const int nb = n_valid ? min(max(n_valid[b], 1), N) : N;
    const int live = (nb + SG_RT - 1) / SG_RT;
    const float* p = part + (size_t)b * tpc * C + c;
    float mx = p[0];
    for (int t = 1; t < live; ++t) mx = fmaxf(mx, p[(size_t)t * C]);
    out[(size_t)b * ldo + c] = mx;
}

// ------------------------------------------------------------------------------------------------------- global
struct SegGlobalArgs {
    float* F; int ldf;
    const int32_t* n_valid; int B, N, tpc;
    const float* TT;                               // [B][128][128]: TT[b][j][k] = T128[b][k][j]
    const float* W[2]; const float* scl[2]; const float* shf[2];
    float slope;
    float* part;                                   // [B * tpc][2048]
};

__global__ __launch_bounds__(SG_T, 1) void seg_global_kernel(const SegGlobalArgs a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* X4 = smem;                              // [RT][LD4]: out4; before it exists, out3 and its transform lie inside
    float* X1 = smem;                              // [RT][LD]
    float* X2 = X1 + SG_RT * SG_LD;                // [RT][LD]
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int t = blockIdx.x / a.B, b = blockIdx.x - t * a.B;
    const int nb = a.n_valid ? min(max(a.n_valid[b], 1), a.N) : a.N;
    const int row0 = t * SG_RT;
    if (row0 >= nb) return;
    const int nrows = min(SG_RT, nb - row0);
    const float* Fb = a.F + (size_t)b * a.N * a.ldf;
    for (int i = tid; i < SG_RT * (SG_C3 / 4); i += SG_T) {
        const int r = i / (SG_C3 / 4), c4 = (i % (SG_C3 / 4)) * 4;
        const float* src = Fb + (size_t)min(row0 + r, a.N - 1) * a.ldf + SG_F3 + c4;
        *reinterpret_cast<float4*>(X1 + r * SG_LD + c4) = *reinterpret_cast<const float4*>(src);
    }
    __syncthreads();
    seg_layer<SG_C3, SG_LD, SG_C3, SG_LD, false>(X1, a.TT + (size_t)b * SG_C3 * SG_C3, nullptr, nullptr, a.slope, X2, nullptr, 0, nrows, wave,
                                                 lane);
    __syncthreads();
    float* Fr = a.F + ((size_t)b * a.N + row0) * a.ldf;
    seg_layer<SG_C3, SG_LD, SG_C4, SG_LD4, true>(X2, a.W[0], a.scl[0], a.shf[0], a.slope, X4, Fr + SG_F4, a.ldf, nrows, wave, lane);
    __syncthreads();
    seg_max_passes<SG_C4, SG_LD4, SG_C5, false>(X4, a.W[1], a.scl[1], a.shf[1], a.slope, nrows, a.part + ((size_t)b * a.tpc + t) * SG_C5, wave,
                                                lane);
}

// ------------------------------------------------------------------------------------------------------- head
struct SegHeadArgs {
    const float* F; int ldf;
    const int32_t* n_valid; int B, N, tpc;
    const float* bias; int ldb;                    // [B][256] per-cloud bias of layer 1 (added before its scale / shift)
    const float* W[4]; const float* scl[3]; const float* shf[3];
    const float* bout; int part_num;
    float slope;
    float* out; size_t ob, oc, on;
};

// columns [k0, k0 + kw) of the tile's rows of F -> buf [RT][LD]
__device__ __forceinline__ void seg_stage(const float* __restrict__ Fb, int ldf, int N, int row0, int k0, int kw, float* buf, int tid) {
    const int per = kw / 4;
    for (int i = tid; i < SG_RT * per; i += SG_T) {
        const int r = i / per, c4 = (i - r * per) * 4;
        const float* src = Fb + (size_t)min(row0 + r, N - 1) * ldf + k0 + c4;
        *reinterpret_cast<float4*>(buf + r * SG_LD + c4) = *reinterpret_cast<const float4*>(src);
    }
}

__global__ __launch_bounds__(SG_T, 2) void seg_head_kernel(const SegHeadArgs a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* Y = smem;                               // [RT][LDH], over the two chunk buffers once layer 1 has read them
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, lr = lane & 31, lh = lane >> 5;
    const int t = blockIdx.x / a.B, b = blockIdx.x - t * a.B;
    const int nb = a.n_valid ? min(max(a.n_valid[b], 1), a.N) : a.N;
    const int row0 = t * SG_RT;
    float* ob = a.out + (size_t)b * a.ob;
    if (row0 >= nb) {                              // a tile of pad rows only: its logits are zeros; nothing is loaded
        if (row0 + lane < a.N)
            for (int c = wave; c < a.part_num; c += 4) ob[(size_t)c * a.oc + (size_t)(row0 + lane) * a.on] = 0.f;
        return;
    }
    const int nrows = min(SG_RT, nb - row0);
    const float* Fb = a.F + (size_t)b * a.N * a.ldf;
    // layer 1: 832 -> 256 over K-chunks of 128 (the last one 64), the next chunk staged while this one is multiplied
    constexpr int NFULL = SG_FK / SG_CHUNK, REST = SG_FK - NFULL * SG_CHUNK;
    static_assert(REST == 64 && NFULL % 2 == 0, "the chunk schedule below");
    f32x16 acc[2][SG_NJ];
#pragma unroll
    for (int rb = 0; rb < 2; ++rb)
#pragma unroll
        for (int j = 0; j < SG_NJ; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[rb][j][r] = 0.f;
    seg_stage(Fb, a.ldf, a.N, row0, 0, SG_CHUNK, smem, tid);
    __syncthreads();
    for (int c = 0; c < NFULL; ++c) {
        const float* cur = smem + (c & 1) * SG_RT * SG_LD;
        float* nxt = smem + ((c + 1) & 1) * SG_RT * SG_LD;
        seg_stage(Fb, a.ldf, a.N, row0, (c + 1) * SG_CHUNK, c + 1 < NFULL ? SG_CHUNK : REST, nxt, tid);
        mfma_layer_acc<SG_CHUNK, SG_LD, SG_NJ, SG_H1 / 32>(cur, a.W[0] + c * SG_CHUNK, SG_FK, wave, lane, acc);
        __syncthreads();
    }
    mfma_layer_acc<REST, SG_LD, SG_NJ, SG_H1 / 32>(smem, a.W[0] + NFULL * SG_CHUNK, SG_FK, wave, lane, acc);
    __syncthreads();
#pragma unroll
    for (int j = 0; j < SG_NJ; ++j) {
        const int col = (wave + 4 * j) * 32 + lr;
        const float sc = a.scl[0][col], sh = a.shf[0][col], cb = a.bias[(size_t)b * a.ldb + col];
#pragma unroll
        for (int rb = 0; rb < 2; ++rb)
#pragma unroll
            for (int r = 0; r < 16; ++r) Y[acc_row(rb, r, lh) * SG_LDH + col] = act(sc * (acc[rb][j][r] + cb) + sh, a.slope);
    }
    __syncthreads();
    seg_layer<SG_H1, SG_LDH, SG_H2, SG_LDH, true>(Y, a.W[1], a.scl[1], a.shf[1], a.slope, Y, nullptr, 0, nrows, wave, lane);
    __syncthreads();
    seg_layer<SG_H2, SG_LDH, SG_H3, SG_LDH, true>(Y, a.W[2], a.scl[2], a.shf[2], a.slope, Y, nullptr, 0, nrows, wave, lane);
    __syncthreads();
    // layer 4: linear + bias on the column blocks that hold a part; W[3] has whole blocks of rows (the launcher checks)
    const int ncb = (a.part_num + 31) / 32;
    f32x16 lo[2][1];
    if (wave < ncb) mfma_layer<SG_H3, SG_LDH, 1, 4>(Y, a.W[3], wave, lane, lo);
    __syncthreads();
    if (wave < ncb) {
        const int col = wave * 32 + lr;
        const float bo = col < a.part_num ? a.bout[col] : 0.f;
#pragma unroll
        for (int rb = 0; rb < 2; ++rb)
#pragma unroll
            for (int r = 0; r < 16; ++r) Y[acc_row(rb, r, lh) * SG_LDH + col] = lo[rb][0][r] + bo;
    }
    __syncthreads();
    // the output's own layout [B, part_num, N]: a wave stores 64 consecutive points of one part; pad points are zeros
    if (row0 + lane < a.N)
        for (int c = wave; c < a.part_num; c += 4)
            ob[(size_t)c * a.oc + (size_t)(row0 + lane) * a.on] = lane < nrows ? Y[lane * SG_LDH + c] : 0.f;
}

// ------------------------------------------------------------------------------------------------------- B-row tails
// y[r][c] = act(scale[c] * (x[r] . W[c]) + shift[c]) (scale null: 1): one wave per column with its weight row in registers, the
// rows four at a time (a row beyond R repeats row R - 1 and is not stored).  Lane l sums its k = 4 (l + 64 i) + e in ascending (i, e), then the lanes are summed by halving: a value does not
// depend on how many rows the call has.
// NV: 16-byte pieces per lane (K <= 256 NV); the narrow layers take the small instantiations and their occupancy.
constexpr int SG_ROWS_V = 9;                       // the widest: K <= 2304
template <int NV>
__global__ __launch_bounds__(SG_T) void seg_rows_kernel(const float* __restrict__ x, int ldx, int R, int K, const float* __restrict__ W,
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

int tiles_of(int N) { return (N + SG_RT - 1) / SG_RT; }

// what every launcher asks of its sizes
int seg_sizes_ok(const char* who, int B, int N) {
    PCL_REQUIRE(B >= 1 && N >= 1, "%s: bad sizes B=%d N=%d", who, B, N);
    PCL_REQUIRE((size_t)B * tiles_of(N) < (1u << 31) / SG_RT, "%s: too many points", who);
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

extern "C" int pcl_pointnet_seg_stn_infer_f32(const float* x, size_t stride_b, size_t stride_n, size_t stride_c, const int32_t* n_valid,
                                              int B, int N, int L, const int32_t* widths, const float* W0, int ldw0, const float* const* W,
                                              const float* const* scale, const float* const* shift, float slope, void* workspace,
                                              size_t workspace_bytes, float* out, int ldo, void* stream) {
    const char* who = "pcl_pointnet_seg_stn_infer_f32";
    PCL_REQUIRE(widths && W && scale && shift, "%s: null host array", who);
    PCL_REQUIRE(seg_shape_ok(PCL_SEG_STN, 3, L, widths), "%s: no kernel for these widths (pcl_pointnet_seg_infer_supported)", who);
    PCL_REQUIRE(x && W0 && out, "%s: null pointer (x, W0 or out)", who);
    if (int rc = seg_sizes_ok(who, B, N)) return rc;
    PCL_REQUIRE(ldw0 >= 3 && ldo >= SG_CT, "%s: ldw0=%d ldo=%d", who, ldw0, ldo);
    for (int l = 0; l < 3; ++l) PCL_REQUIRE(scale[l] && shift[l] && (l == 0 || W[l]), "%s: layer %d: null pointer", who, l);
    if (int rc = seg_part_ok(who, workspace, workspace_bytes, B, N, SG_CT)) return rc;
    PCL_REQUIRE(al16(W[1], W[2]), "%s: the weights of layers 2-3 must be 16-byte aligned", who);
    SegFrontArgs a = {};
    a.x = x; a.sb = stride_b; a.sn = stride_n; a.sc = stride_c;
    a.n_valid = n_valid; a.B = B; a.N = N; a.tpc = tiles_of(N);
    a.W0 = W0; a.ldw0 = ldw0;
    for (int l = 0; l < 3; ++l) { a.sW[l] = W[l]; a.sscl[l] = scale[l]; a.sshf[l] = shift[l]; }
    a.slope = slope;
    a.part = static_cast<float*>(workspace);
    hipStream_t st = as_stream(stream);
    if (int rc = lds_opt_in(seg_front_kernel<false>, SG_LDS_FRONT, who)) return rc;
    hipLaunchKernelGGL(seg_front_kernel<false>, dim3(B * a.tpc), dim3(SG_T), SG_LDS_FRONT, st, a);
    if (int rc = check_launch(who)) return rc;
    hipLaunchKernelGGL(seg_tile_max_kernel, dim3(B, SG_CT / SG_T), dim3(SG_T), 0, st, a.part, n_valid, N, a.tpc, SG_CT, out, ldo);
    return check_launch(who);
}

extern "C" int pcl_pointnet_seg_trunk_infer_f32(const float* x, size_t stride_b, size_t stride_n, size_t stride_c, const int32_t* n_valid,
                                                int B, int N, const float* T3, int L, const int32_t* widths, const float* W0, int ldw0,
                                                const float* const* W, const float* const* scale, const float* const* shift, int Ls,
                                                const int32_t* widths_s, const float* const* Ws, const float* const* scale_s,
                                                const float* const* shift_s, float slope, float* F, int ldf, size_t f_bytes,
                                                void* workspace, size_t workspace_bytes, float* out, int ldo, void* stream) {
    const char* who = "pcl_pointnet_seg_trunk_infer_f32";
    PCL_REQUIRE(widths && W && scale && shift && widths_s && Ws && scale_s && shift_s, "%s: null host array", who);
    PCL_REQUIRE(seg_shape_ok(PCL_SEG_TRUNK, 3, L, widths) && seg_shape_ok(PCL_SEG_FSTN, SG_C3, Ls, widths_s),
                "%s: no kernel for these widths (pcl_pointnet_seg_infer_supported)", who);
    PCL_REQUIRE(x && T3 && W0 && out, "%s: null pointer (x, T3, W0 or out)", who);
    if (int rc = seg_sizes_ok(who, B, N)) return rc;
    PCL_REQUIRE(ldw0 >= 3 && ldo >= SG_CT, "%s: ldw0=%d ldo=%d", who, ldw0, ldo);
    for (int l = 0; l < 3; ++l)
        PCL_REQUIRE(scale[l] && shift[l] && (l == 0 || W[l]) && scale_s[l] && shift_s[l] && Ws[l], "%s: layer %d: null pointer", who, l);
    if (int rc = seg_rows_ok(who, F, ldf, f_bytes, B, N)) return rc;
    if (int rc = seg_part_ok(who, workspace, workspace_bytes, B, N, SG_CT)) return rc;
    PCL_REQUIRE(al16(W[1], W[2], Ws[0], Ws[1], Ws[2]), "%s: the weights of the MFMA layers must be 16-byte aligned", who);
    SegFrontArgs a = {};
    a.x = x; a.sb = stride_b; a.sn = stride_n; a.sc = stride_c;
    a.n_valid = n_valid; a.B = B; a.N = N; a.tpc = tiles_of(N);
    a.T3 = T3; a.W0 = W0; a.ldw0 = ldw0;
    for (int l = 0; l < 3; ++l) {
        a.cW[l] = W[l]; a.cscl[l] = scale[l]; a.cshf[l] = shift[l];
        a.sW[l] = Ws[l]; a.sscl[l] = scale_s[l]; a.sshf[l] = shift_s[l];
    }
    a.slope = slope;
    a.F = F; a.ldf = ldf;
    a.part = static_cast<float*>(workspace);
    hipStream_t st = as_stream(stream);
    if (int rc = lds_opt_in(seg_front_kernel<true>, SG_LDS_FRONT, who)) return rc;
    hipLaunchKernelGGL(seg_front_kernel<true>, dim3(B * a.tpc), dim3(SG_T), SG_LDS_FRONT, st, a);
    if (int rc = check_launch(who)) return rc;
    hipLaunchKernelGGL(seg_tile_max_kernel, dim3(B, SG_CT / SG_T), dim3(SG_T), 0, st, a.part, n_valid, N, a.tpc, SG_CT, out, ldo);
    return check_launch(who);
}

extern "C" int pcl_pointnet_seg_global_infer_f32(float* F, int ldf, size_t f_bytes, const int32_t* n_valid, int B, int N, const float* TT,
                                                 int L, const int32_t* widths, const float* const* W, const float* const* scale,
                                                 const float* const* shift, float slope, void* workspace, size_t workspace_bytes,
                                                 float* out, int ldo, void* stream) {
    const char* who = "pcl_pointnet_seg_global_infer_f32";
    PCL_REQUIRE(widths && W && scale && shift, "%s: null host array", who);
    PCL_REQUIRE(seg_shape_ok(PCL_SEG_GLOBAL, SG_C3, L, widths), "%s: no kernel for these widths (pcl_pointnet_seg_infer_supported)", who);
    PCL_REQUIRE(TT && out, "%s: null pointer (TT or out)", who);
    if (int rc = seg_sizes_ok(who, B, N)) return rc;
    PCL_REQUIRE(ldo >= SG_C5, "%s: ldo=%d", who, ldo);
    for (int l = 0; l < 2; ++l) PCL_REQUIRE(scale[l] && shift[l] && W[l], "%s: layer %d: null pointer", who, l);
    if (int rc = seg_rows_ok(who, F, ldf, f_bytes, B, N)) return rc;
    if (int rc = seg_part_ok(who, workspace, workspace_bytes, B, N, SG_C5)) return rc;
    PCL_REQUIRE(al16(TT, W[0], W[1]), "%s: TT and the weights must be 16-byte aligned", who);
    SegGlobalArgs a = {};
    a.F = F; a.ldf = ldf;
    a.n_valid = n_valid; a.B = B; a.N = N; a.tpc = tiles_of(N);
    a.TT = TT;
    for (int l = 0; l < 2; ++l) { a.W[l] = W[l]; a.scl[l] = scale[l]; a.shf[l] = shift[l]; }
    a.slope = slope;
    a.part = static_cast<float*>(workspace);
    hipStream_t st = as_stream(stream);
    if (int rc = lds_opt_in(seg_global_kernel, SG_LDS_GLOBAL, who)) return rc;
    hipLaunchKernelGGL(seg_global_kernel, dim3(B * a.tpc), dim3(SG_T), SG_LDS_GLOBAL, st, a);
    if (int rc = check_launch(who)) return rc;
    hipLaunchKernelGGL(seg_tile_max_kernel, dim3(B, SG_C5 / SG_T), dim3(SG_T), 0, st, a.part, n_valid, N, a.tpc, SG_C5, out, ldo);
    return check_launch(who);
}

extern "C" int pcl_pointnet_seg_head_infer_f32(const float* F, int ldf, size_t f_bytes, const int32_t* n_valid, int B, int N,
                                               const float* cloud_bias, int ldb, int L, const int32_t* widths, const float* const* W,
                                               int w_out_rows, const float* const* scale, const float* const* shift, const float* bias_out,
                                               float slope, float* out, size_t stride_b, size_t stride_c, size_t stride_n, void* stream) {
    const char* who = "pcl_pointnet_seg_head_infer_f32";
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
    PCL_REQUIRE(al16(W[0], W[1], W[2], W[3]), "%s: the weights must be 16-byte aligned", who);
    SegHeadArgs a = {};
    a.F = F; a.ldf = ldf;
    a.n_valid = n_valid; a.B = B; a.N = N; a.tpc = tiles_of(N);
    a.bias = cloud_bias; a.ldb = ldb;
    for (int l = 0; l < 4; ++l) a.W[l] = W[l];
    for (int l = 0; l < 3; ++l) { a.scl[l] = scale[l]; a.shf[l] = shift[l]; }
    a.bout = bias_out; a.part_num = part_num;
    a.slope = slope;
    a.out = out; a.ob = stride_b; a.oc = stride_c; a.on = stride_n;
    hipStream_t st = as_stream(stream);
    if (int rc = lds_opt_in(seg_head_kernel, SG_LDS_HEAD, who)) return rc;
    hipLaunchKernelGGL(seg_head_kernel, dim3(B * a.tpc), dim3(SG_T), SG_LDS_HEAD, st, a);
    return check_launch(who);
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
    const dim3 grid((C + 3) / 4), block(SG_T);
    if (K <= 256) hipLaunchKernelGGL(seg_rows_kernel<1>, grid, block, 0, st, x, ldx, R, K, W, scale, shift, slope, y, ldy, C);
    else if (K <= 1024) hipLaunchKernelGGL(seg_rows_kernel<4>, grid, block, 0, st, x, ldx, R, K, W, scale, shift, slope, y, ldy, C);
    else hipLaunchKernelGGL(seg_rows_kernel<SG_ROWS_V>, grid, block, 0, st, x, ldx, R, K, W, scale, shift, slope, y, ldy, C);
    return check_launch(who);
}
