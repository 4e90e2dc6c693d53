// infer_pointnet.hip -- the PointNet conv stack and its max over the points in evaluation mode (networks/cls/pointnet.py:28-36
// under net.eval(), as train_cls.py:92-124 evaluates it): conv/bn/relu x 5 (3 -> 64 -> 64 -> 64 -> 128 -> 1024) and the max over
// each cloud's points, with no activation written to memory.
//
//     z_1 = act(scale_1 * (W0 x) + shift_1),  z_l = act(scale_l * (W_l z_{l-1}) + shift_l) (l >= 2),
//     out[b*ldo + c] = max over i < n_b of z_5[b, i, c]
//
// A workgroup (4 waves) owns one 64-row tile of ONE cloud (tiles never span clouds) and, with `splits` column splits of the last
// layer over grid.y, 1024 / splits of its columns:
//   1. layer 1 (K = 3) elementwise from the three coordinates, read at the caller's strides ([B,3,N] or [B,N,3] as it is),
//      four channels per thread -> X1 (LDS) (infer::points_layer);
//   2. layers 2-4 on the fp32 MFMA (infer::tile_layer), ping-ponging between X1 and X2, two [64][132] fp32 tiles in LDS;
//   3. layer 5 (128 -> 1024, 89 % of the FLOPs) in passes of 256 columns (infer::max_passes; 64 accumulator registers, no scratch):
//      scale / shift / act in the epilogue, rows >= n_b selected to -inf, the max over the lane's 32 rows in registers, then
//      across the two lane halves; z_5 reaches neither LDS nor memory.  Lane half 0 stores the tile's partial maxima
//      part[tile][col] (the caller's workspace).
// A tile whose first row is >= n_b leaves before any load; its partials are never read, so the workspace is never cleared.
// Workgroups are numbered tile-major (blockIdx.x = t * B + b, infer::cloud_tile): the tiles that ragged clouds leave empty are
// the high t of every cloud, and dispatched last they cost next to nothing; numbered cloud by cloud, interleaved with live
// tiles, each empty workgroup was measured to cost nearly what a live one does.  A
// partial tile computes all 64 rows: rows of a GEMM are independent, so whatever a pad row holds (NaN included) stays in that row.
// Rows beyond the capacity N repeat row N - 1 (never read out of bounds) and are masked like every row >= n_b.
// A second small launch (infer::tile_max_kernel) takes, per cloud and column, the max over the cloud's ceil(n_b / 64) live tiles
// in ascending order.  No atomics and no inter-workgroup hand-off inside a launch.
//
// With a split, layers 1-4 (11 % of the FLOPs) are recomputed per split.  splits = pcl_pointnet_stack_infer_splits(B, N), a pure
// function of the sizes: few tiles (B = 8, N = 1024: 128 for 256 CUs) take 4 or 2 splits to fill the machine.
//
// Numerics: layer 1 is fmaf(w2, z, fmaf(w1, y, w0 * x)); layers 2-5 are fp32 products accumulated in fp32 in the k order of
// infer::mfma_layer; epilogues are scale * y + shift (two roundings) and the leaky ReLU; max is exact.  Every column's value is
// computed by the same instruction sequence in every variant, tiles are cut from the cloud's own first row and reduced in
// ascending order: a cloud's output depends only on its own valid rows -- bit for bit the same for any B, any position in the
// batch, any capacity N, any pad contents, any number of splits and any run.
//
// The bf16 kernel (pcl_pointnet_stack_infer_bf16_f32, pointnet_stack_infer_bf16_kernel) keeps that geometry -- one workgroup per
// row tile of one cloud, tile-major, the early exit, per-tile partials in the never-cleared workspace, the same second launch, the
// same splits, no atomics -- with layers 2-5 on v_mfma_f32_32x32x16_bf16 (infer::mfma_layer_bf16) and X1 / X2 as [rows][K + 8]
// bf16 tiles.  Numerics contract (mirrors pcl_sa_level_infer_bf16_f32, infer.hip):
//   - layer 1 is the fp32 fmaf expression above with its epilogue in fp32; z_1 is rounded to nearest even to bf16 ((__bf16));
//   - layers 2-5 are bf16 x bf16 products accumulated in fp32, k-blocks of 16 in ascending order; every epilogue
//     act(scale * y + shift) runs in fp32; z_2 .. z_4 are rounded to nearest even to bf16;
//   - z_5 is never rounded; the max, the partials and out are fp32; W0, scale and shift stay fp32;
//   - a cloud's output depends only on its own valid rows: the same bits for any B, position, capacity N, pad contents, split
//     count, rows per workgroup and run.
// Two things differ from the fp32 kernel's shape, both sized in DESIGN.md section 21:
//   - the layer-5 epilogue runs on the tile's extreme raw accumulators, not on every element: for 0 <= slope <= 1 (checked on the
//     host) u -> act(fl(fl(scale * u) + shift)) is monotone because fp32 rounding is, non-decreasing for scale >= 0 and
//     non-increasing for scale < 0, so the max over rows of the epilogue IS the epilogue of the max (scale >= 0) or the min
//     (scale < 0) of the accumulators, bit for bit.  Rows >= n_b are selected out of both (a pad row may hold anything);
//   - a workgroup may take 128 rows (four 32-row blocks per weight piece: half the weight bytes per row from L2); it stores the
//     same partial into both of its 64-row slots (max is idempotent), so the second launch and the workspace layout are shared.
#include "common.h"
#include "infer_mfma.h"

namespace pcl {
namespace {

using namespace infer;

constexpr int PN_C0 = 3, PN_C1 = 64, PN_C2 = 64, PN_C3 = 64, PN_C4 = 128, PN_C5 = 1024;
constexpr size_t PN_LDS = 4 * (size_t)2 * RT * LD128;                    // X1 and X2, 67 584 B: two workgroups per CU

struct PnArgs {
    const float* x; size_t sb, sn, sc;
    const int32_t* n_valid; int B, N, tpc;         // tpc: tiles per cloud = ceil(N / 64)
    const float* W0; int ldw0;
    const float* W[5]; const float* scl[5]; const float* shf[5];
    float slope;
    float* part;                                   // [B * tpc][1024]
    int cols_per_split;
};

__global__ __launch_bounds__(NT, 2) void pointnet_stack_infer_kernel(const PnArgs a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* X1 = smem;                              // [RT][LD128]
    float* X2 = X1 + RT * LD128;                   // [RT][LD128]
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const CloudTile tile = cloud_tile<RT>(a.B, a.N, a.n_valid);
    if (tile.empty()) return;
    // 1. layer 1: a thread always works on the same four channels
    points_layer<float, RT, LD128, false, false>(a.x + (size_t)tile.b * a.sb, a.sn, a.sc, a.N, tile.row0, nullptr, a.W0, a.ldw0, a.scl[0],
                                                 a.shf[0], a.slope, X1, nullptr, 0, tile.nrows, tid);
    __syncthreads();
    // 2. layers 2-4
    tile_layer<PN_C1, LD128, PN_C2, LD128>(X1, a.W[1], a.scl[1], a.shf[1], a.slope, X2, wave, lane);
    __syncthreads();
    tile_layer<PN_C2, LD128, PN_C3, LD128>(X2, a.W[2], a.scl[2], a.shf[2], a.slope, X1, wave, lane);
    __syncthreads();
    tile_layer<PN_C3, LD128, PN_C4, LD128>(X1, a.W[3], a.scl[3], a.shf[3], a.slope, X2, wave, lane);
    __syncthreads();
    // 3. layer 5 over this split's columns; the max over the tile's rows in registers
    float* part = a.part + ((size_t)tile.b * a.tpc + tile.t) * PN_C5;
    const int c_begin = blockIdx.y * a.cols_per_split;
    max_passes<PN_C4, LD128, true>(X2, a.W[4], a.scl[4], a.shf[4], a.slope, tile.nrows, part, c_begin, c_begin + a.cols_per_split, wave, lane);
}

// ------------------------------------------------------------------------------------------------- the bf16 instantiation
// X1 holds z_1 / z_3 (64 wide), X2 z_2 (64) then z_4 (128): [rows][K + 8] bf16
constexpr int PN16_LD1 = PN_C1 + row_pad<__bf16>, PN16_LD4 = PN_C4 + row_pad<__bf16>;
constexpr size_t pn16_lds(int nrb) { return 2 * (size_t)32 * nrb * (PN16_LD1 + PN16_LD4); }   // 26 624 B (64 rows), 53 248 B (128)

// NRB: 32-row blocks per workgroup (2 or 4)
template <int NRB>
__global__ __launch_bounds__(NT, 2) void pointnet_stack_infer_bf16_kernel(const PnArgs a) {
    constexpr int ROWS = 32 * NRB;
    constexpr int NJ5 = 4 / NRB, PASS5 = 4 * NJ5 * 32;   // layer 5: 64 accumulator registers either way, passes of 256 / 128 columns
    extern __shared__ __attribute__((aligned(16))) float smem[];
    __bf16* X1 = reinterpret_cast<__bf16*>(smem);  // [ROWS][LD1]
    __bf16* X2 = X1 + ROWS * PN16_LD1;             // [ROWS][LD4] (z_2 at stride LD1)
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, lr = lane & 31, lh = lane >> 5;
    const CloudTile tile = cloud_tile<ROWS>(a.B, a.N, a.n_valid);
    if (tile.empty()) return;
    // 1. layer 1 in fp32, rounded into the bf16 tile
    points_layer<__bf16, ROWS, PN16_LD1, false, false>(a.x + (size_t)tile.b * a.sb, a.sn, a.sc, a.N, tile.row0, nullptr, a.W0, a.ldw0, a.scl[0],
                                                       a.shf[0], a.slope, X1, nullptr, 0, tile.nrows, tid);
    __syncthreads();
    // 2. layers 2-4
    tile_layer<PN_C1, PN16_LD1, PN_C2, PN16_LD1, NRB>(X1, a.W[1], a.scl[1], a.shf[1], a.slope, X2, wave, lane);
    __syncthreads();
    tile_layer<PN_C2, PN16_LD1, PN_C3, PN16_LD1, NRB>(X2, a.W[2], a.scl[2], a.shf[2], a.slope, X1, wave, lane);
    __syncthreads();
    tile_layer<PN_C3, PN16_LD1, PN_C4, PN16_LD4, NRB>(X1, a.W[3], a.scl[3], a.shf[3], a.slope, X2, wave, lane);
    __syncthreads();
    // 3. layer 5 in passes; the workgroup's 64-row slots of the partials both take its maxima
    float* part = a.part + ((size_t)tile.b * a.tpc + tile.t * (ROWS / RT)) * PN_C5;
    const bool second = ROWS > RT && tile.row0 + RT < tile.nb;
    const bool full = tile.nrows == ROWS;
    const int c_begin = blockIdx.y * a.cols_per_split, c_end = c_begin + a.cols_per_split;
    for (int c0 = c_begin; c0 < c_end; c0 += PASS5) {
        f32x16 acc[NRB][NJ5];
        mfma_layer_bf16<PN_C4, PN16_LD4, NJ5, 4 * NJ5, NRB>(X2, reinterpret_cast<const __bf16*>(a.W[4]) + (size_t)c0 * PN_C4, wave, lane,
                                                                 acc);
#pragma unroll
        for (int j = 0; j < NJ5; ++j) {
            const int col = c0 + (wave + 4 * j) * 32 + lr;
            const float sc = a.scl[4][col], sh = a.shf[4][col];
            float mx = -INFINITY, mn = INFINITY;   // the extreme accumulators of the tile's valid rows (header comment)
            if (full) {
#pragma unroll
                for (int rb = 0; rb < NRB; ++rb)
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        mx = fmaxf(mx, acc[rb][j][r]);
                        mn = fminf(mn, acc[rb][j][r]);
                    }
            } else {
#pragma unroll
                for (int rb = 0; rb < NRB; ++rb)
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const bool ok = acc_row(rb, r, lh) < tile.nrows;
                        mx = fmaxf(mx, ok ? acc[rb][j][r] : -INFINITY);
                        mn = fminf(mn, ok ? acc[rb][j][r] : INFINITY);
                    }
            }
            mx = fmaxf(mx, __shfl_xor(mx, 32));
            mn = fminf(mn, __shfl_xor(mn, 32));
            mx = act(sc * (sc >= 0.f ? mx : mn) + sh, a.slope);
            if (lh == 0) {
                part[col] = mx;
                if (second) part[PN_C5 + col] = mx;
            }
        }
    }
}

// Rows per workgroup of the bf16 kernel, a pure function of the sizes: 128 once there is a 128-row tile for each of the MI355X's
// 256 CUs, else 64 (measured either side of it).  The result's bits do not depend on it.
int pn16_rows(int B, int N) { return (long long)B * ((N + 127) / 128) >= 256 ? 128 : 64; }

bool pn_shape_ok(int C0, int L, const int32_t* w) {
    return C0 == PN_C0 && L == 5 && w && w[0] == PN_C1 && w[1] == PN_C2 && w[2] == PN_C3 && w[3] == PN_C4 && w[4] == PN_C5;
}

}  // namespace
}  // namespace pcl
using namespace pcl;

extern "C" int pcl_pointnet_stack_infer_supported(int C0, int L, const int32_t* widths) { return pn_shape_ok(C0, L, widths); }

extern "C" size_t pcl_pointnet_stack_infer_workspace_bytes(int B, int N, int C_last) {
    if (B < 1 || N < 1 || C_last < 1) return 0;
    return 4 * (size_t)B * ((N + RT - 1) / RT) * C_last;
}

// 512 workgroups are two per CU of the MI355X's 256: fewer tiles than that split the last layer's columns
extern "C" int pcl_pointnet_stack_infer_splits(int B, int N) {
    if (B < 1 || N < 1) return 1;
    const long long tiles = (long long)B * ((N + RT - 1) / RT);
    return tiles <= 128 ? 4 : tiles <= 256 ? 2 : 1;
}

namespace {

template <int NRB>
int pn16_launch(const char* who, const PnArgs& a, int splits, hipStream_t st) {
    auto kern = pointnet_stack_infer_bf16_kernel<NRB>;
    const int tiles = (a.N + 32 * NRB - 1) / (32 * NRB);
    if (int rc = lds_opt_in(kern, pn16_lds(NRB), who)) return rc;
    hipLaunchKernelGGL(kern, dim3(a.B * tiles, splits), dim3(NT), pn16_lds(NRB), st, a);
    return check_launch(who);
}

// both precisions: every check runs before any HIP call.  W[l], l >= 1: fp32 (BF16 false) or bf16 (true) [C_l][C_{l-1}]
template <bool BF16>
int pn_stack_infer(const char* who, const float* x, size_t stride_b, size_t stride_n, size_t stride_c, const int32_t* n_valid, int B, int N,
                   int C0, const float* W0, int ldw0, int L, const int32_t* widths, const void* const* W, const float* const* scale,
                   const float* const* shift, float slope, void* workspace, size_t workspace_bytes, float* out, int ldo, void* stream) {
    PCL_REQUIRE(widths && W && scale && shift, "%s: null host array", who);
    PCL_REQUIRE(L >= 1 && L <= 5, "%s: L=%d", who, L);
    PCL_REQUIRE(pn_shape_ok(C0, L, widths), "%s: no kernel for C0=%d L=%d widths %d/%d/%d/%d/%d (pcl_pointnet_stack_infer_supported)", who,
                C0, L, widths[0], L > 1 ? widths[1] : 0, L > 2 ? widths[2] : 0, L > 3 ? widths[3] : 0, L > 4 ? widths[4] : 0);
    PCL_REQUIRE(x && W0 && out, "%s: null pointer (x, W0 or out)", who);
    PCL_REQUIRE(B >= 1 && N >= 1, "%s: bad sizes B=%d N=%d", who, B, N);
    const int tpc = (N + RT - 1) / RT;
    PCL_REQUIRE((size_t)B * tpc < (1u << 31) / RT, "%s: too many points", who);
    PCL_REQUIRE(ldw0 >= PN_C0 && ldo >= PN_C5, "%s: ldw0=%d ldo=%d for %d -> %d channels", who, ldw0, ldo, PN_C0, PN_C5);
    for (int l = 0; l < L; ++l) PCL_REQUIRE(scale[l] && shift[l] && (l == 0 || W[l]), "%s: layer %d: null pointer", who, l);
    // the bf16 kernel's last epilogue runs on the extreme accumulators: monotone only for these slopes (header comment)
    if (BF16) PCL_REQUIRE(slope >= 0.f && slope <= 1.f, "%s: slope %g outside [0, 1]", who, (double)slope);
    const size_t need = pcl_pointnet_stack_infer_workspace_bytes(B, N, PN_C5);
    if (!workspace || workspace_bytes < need) return fail(PCL_EWS, "%s: workspace %zu < %zu", who, workspace_bytes, need);
    bool aligned = al16(workspace);
    for (int l = 1; l < L; ++l) aligned = aligned && al16(W[l]);
    PCL_REQUIRE(aligned, "%s: the weights of layers 2-5 and the workspace must be 16-byte aligned", who);
    PnArgs a = {};
    a.x = x; a.sb = stride_b; a.sn = stride_n; a.sc = stride_c;
    a.n_valid = n_valid; a.B = B; a.N = N; a.tpc = tpc;
    a.W0 = W0; a.ldw0 = ldw0;
    for (int l = 0; l < L; ++l) { a.W[l] = static_cast<const float*>(W[l]); a.scl[l] = scale[l]; a.shf[l] = shift[l]; }
    a.slope = slope;
    a.part = static_cast<float*>(workspace);
    const int splits = pcl_pointnet_stack_infer_splits(B, N);
    a.cols_per_split = PN_C5 / splits;
    static_assert(PN_C5 / 4 % MAX_PASS == 0, "a split is a whole number of passes");
    hipStream_t st = as_stream(stream);
    if constexpr (BF16) {
        if (int rc = pn16_rows(B, N) == 128 ? pn16_launch<4>(who, a, splits, st) : pn16_launch<2>(who, a, splits, st)) return rc;
    } else {
        if (int rc = lds_opt_in(pointnet_stack_infer_kernel, PN_LDS, who)) return rc;
        hipLaunchKernelGGL(pointnet_stack_infer_kernel, dim3(B * tpc, splits), dim3(NT), PN_LDS, st, a);
        if (int rc = check_launch(who)) return rc;
    }
    hipLaunchKernelGGL(tile_max_kernel<PN_C5>, dim3(B, PN_C5 / NT), dim3(NT), 0, st, static_cast<const float*>(workspace), n_valid, N, tpc,
                       out, ldo);
    return check_launch(who);
}

}  // namespace

extern "C" int pcl_pointnet_stack_infer_f32(const float* x, size_t stride_b, size_t stride_n, size_t stride_c, const int32_t* n_valid,
                                            int B, int N, int C0, const float* W0, int ldw0, int L, const int32_t* widths,
                                            const float* const* W, const float* const* scale, const float* const* shift, float slope,
                                            void* workspace, size_t workspace_bytes, float* out, int ldo, void* stream) {
    return pn_stack_infer<false>("pcl_pointnet_stack_infer_f32", x, stride_b, stride_n, stride_c, n_valid, B, N, C0, W0, ldw0, L, widths,
                                 reinterpret_cast<const void* const*>(W), scale, shift, slope, workspace, workspace_bytes, out, ldo, stream);
}

extern "C" int pcl_pointnet_stack_infer_bf16_f32(const float* x, size_t stride_b, size_t stride_n, size_t stride_c, const int32_t* n_valid,
                                                 int B, int N, int C0, const float* W0, int ldw0, int L, const int32_t* widths,
                                                 const void* const* W, const float* const* scale, const float* const* shift, float slope,
                                                 void* workspace, size_t workspace_bytes, float* out, int ldo, void* stream) {
    return pn_stack_infer<true>("pcl_pointnet_stack_infer_bf16_f32", x, stride_b, stride_n, stride_c, n_valid, B, N, C0, W0, ldw0, L, widths,
                                W, scale, shift, slope, workspace, workspace_bytes, out, ldo, stream);
}
