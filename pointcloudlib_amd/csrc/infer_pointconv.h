// infer_pointconv.h -- the kernel of infer_pointconv.hip and infer_pointconv_seg_bf16.hip (which instantiate it) and its launch:
// one k-NN PointConv level in evaluation mode, up to and including the density-weighted contraction, as ONE
// launch (misc/pointconv_utils.py:361-394 under net.eval()): the folded first layer of the feature MLP, its two 1x1 convs, eval
// BatchNorm + activation after each, the WeightNet (3 -> 8 -> 8 -> 16) and the DensityNet (1 -> 8 -> 8 -> 1) of every row, and
//     out[g, c*16 + m] = sum_s z3[s, c] * rho[s] * w[s, m].
// It is infer.hip's level kernel with the max epilogue replaced by that contraction.  Neither the [B,S,ns,C] activations nor the
// [B,S,ns,16] weights, the [B,N,1] density scale or any gathered tensor exist in memory.
//
// A workgroup (4 waves) owns GT consecutive groups (GT a multiple of the groups per tile) and walks them in tiles of 64 rows: two
// groups per tile at ns = 32, one at ns = 64.  k-NN lists: every slot is a real row.  Per tile:
//   1. row records (tid < 64): source point src = b*N + idx[g, s] (b = g / m; idx clamped to [0, N - 1] as in infer.hip, so that no
//      load leaves the cloud -- the header makes idx in [0, N) the caller's precondition), d = xyz[src] - new_xyz[g] (__fsub_rn),
//      density[src]; a tile's rows beyond the workgroup's last group repeat its last row (their results are never read);
//   2. layer 1 elementwise, four channels per thread: y1 = fmaf chain Wx d + Uf[src], z1 = act(scale1 y1 + shift1) -> X1 (LDS);
//      and, four threads per row, the two small nets from constants staged in LDS once per workgroup: fp32 fmaf chains with k
//      ascending from the first product, relu(scale * y + shift) after each layer; rw[s][m] = rho[s] * w[s][m] -> RW [64][16] (LDS);
//   3. layer 2 on v_mfma_f32_32x32x2_f32 (infer_mfma.h: A from X1, B from the weights in L2) -> z2 -> X2 (LDS);
//   4. layer 3 the same from X2; a barrier (every wave is done reading X2); z3 = act(scale3 y3 + shift3) -> Z [64][C3 + 16] (LDS),
//      which lies over X1 and X2, both dead by then;
//   5. the contraction on v_mfma_f32_16x16x4_f32, the MFMA form: out^T[m, c] = sum_s rw[s, m] Z[s, c].  A = RW^T (lane l: row s0 +
//      (l >> 4), m = l & 15), B = Z (row s0 + (l >> 4), column c0 + (l & 15)), s ascending in steps of 4.  A wave owns four 16-column
//      blocks of one group (four independent accumulators over one A operand); lane l ends with out[g][(c0 + (l & 15)) * 16 +
//      4 (l >> 4) + 0..3]: one 16-byte store, a wave's stores cover 1 KB of the output row without gaps.
// LDS banks (ds_read_b32: (a / 4) % 32 inside a 32-lane half): a half reads two rows of Z, 16 consecutive columns each; with the
// row stride C3 + 16 = 16 (mod 32) floats they fall on the two halves of the banks.  RW rows are 16 floats: a half reads 32
// consecutive floats.  The deposit writes one row's 32 consecutive columns per half.  No conflicts in either direction.
//
// Numeric contract (include/pcl_hip.h): a group's result depends only on its own rows (not on B, on the group's place in the
// launch or on GT); no atomics, two calls give identical bits; out is fully defined for every group.
//
// The kernel is templated on the tile's element type as infer.hip's is.  The bf16 instantiation (pcl_pointconv_level_infer_bf16_f32)
// holds X1 / X2 as bf16 (rows of C + 8 elements: an odd number of 16-byte pieces, infer_mfma.h) and runs layers 2 and 3 on
// v_mfma_f32_32x32x16_bf16, k-blocks of 16 ascending: z1 and z2 are rounded to nearest even when they are stored, W[1] and W[2] are
// bf16; row records, layer 1, the small nets, rw, every epilogue, Z (z3, never rounded) and the contraction are the fp32 text
// above.  Z is larger than X1 | X2 of either element type, so tile_bytes, the place of RW and the LDS totals are those of the fp32
// form, and the barrier in front of the deposit guards the same overlay.
// Layer 1 of this form is written in single-lane steps (lone(), below).
//
// The kernel is also templated on the feature MLP's layer count L (pcl_pointconv_seg_level_infer_f32: the levels of
// networks/seg/pointconv_partseg.py).  L = 2 has no step 3: the last layer reads X1, and Z lies over X1 behind the same barrier.
// The part-seg shapes have the bf16 form too (pcl_pointconv_seg_level_infer_bf16_f32): at L = 2 only z1 is rounded and the one
// MFMA layer reads the bf16 X1.  At 128/128/128 the bf16 X1 | X2 (34 816 B) is smaller than Z (36 864 B), so tile_bytes is Z's and
// that kernel's LDS total drops from 74 816 B to 44 096 B; every other shape keeps the total of its fp32 form.
// At ns = 16 a tile holds four groups and a wave owns all C3 / 16 column blocks of one of them in step 5 (8 or 16 accumulators);
// a tile with 1, 2 or 3 live groups leaves the other waves out of step 5 (gi < ngt).  A layer of 32 columns is one column block:
// waves 1 - 3 idle in it.
#pragma once
#include <type_traits>

#include "common.h"
#include "infer_mfma.h"

namespace pcl {
namespace pointconv {

using namespace infer;

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int PC_M = 16;                           // WeightNet(3, 16)
constexpr int PC_MAXTILES = 8;                     // tiles per workgroup at most
constexpr size_t PC_LDS_CAP = 80 * 1024;           // two workgroups per CU
constexpr int PC_NETS = PCL_POINTCONV_NETS_FLOATS;
// offsets into the packed constants (include/pcl_hip.h documents them)
constexpr int WN_W1 = 0, WN_S1 = 24, WN_T1 = 32, WN_W2 = 40, WN_S2 = 104, WN_T2 = 112, WN_W3 = 120, WN_S3 = 248, WN_T3 = 264;
constexpr int DN_W1 = 280, DN_S1 = 288, DN_T1 = 296, DN_W2 = 304, DN_S2 = 368, DN_T2 = 376, DN_W3 = 384, DN_S3 = 392, DN_T3 = 393;
static_assert(DN_T3 < PC_NETS, "packed constants");

struct PointConvArgs {
    const float* xyz; const float* new_xyz; const float* Uf; const float* Wx; int ldw;
    const float* density; const int32_t* idx;
    int G, N, m, GT;
    const float* W2; const float* W3;
    const float* sc1; const float* sh1; const float* sc2; const float* sh2; const float* sc3; const float* sh3;
    float slope;
    const float* nets;
    float* out; int ldo;
};

// L: layers of the feature MLP (3: C1 -> C2 -> C3; 2: C1 -> C3, C2 is not used and there is no X2)
template <int L, int C1, int C2, int C3, bool BF16>
struct PointConvShape {
    static_assert(L == 2 || L == 3, "layers of the feature MLP");
    using XT = std::conditional_t<BF16, __bf16, float>;                    // element of X1 / X2
    static constexpr int LD1 = C1 + row_pad<XT>, LD2 = C2 + row_pad<XT>, LDZ = C3 + 16;
    static constexpr size_t x_bytes = sizeof(XT) * ((size_t)RT * LD1 + (L == 3 ? RT * LD2 : 0));
    static constexpr size_t tile_bytes = x_bytes > 4 * (size_t)RT * LDZ ? x_bytes : 4 * (size_t)RT * LDZ;
    // X1 | X2 under Z, RW, row records (d, src, density), the small nets' constants
    static constexpr size_t lds_bytes = tile_bytes + 4 * (size_t)RT * PC_M + 16 * RT + 4 * RT + 4 * RT + 4 * PC_NETS;
    static_assert(lds_bytes <= PC_LDS_CAP, "two workgroups per CU");
};

__device__ __forceinline__ float relu_bn(float y, float sc, float sh) { return fmaxf(sc * y + sh, 0.f); }

// Keeps a value out of the packed two-channel fp32 instructions (v_pk_fma_f32, v_pk_mul_f32, v_pk_add_f32) that the compiler
// otherwise forms from a thread's four layer-1 channels.  In the 128/128/256 bf16 kernel, with two workgroups on a compute unit, a
// chain of such instructions two apart now and then lost one step in the low channel of lanes 48 - 63 (dumps of X1: the y term of
// layer 1 missing from channels 4k or 4k + 2 >= 64 of one odd row, 2 to 9 groups of 4101 in a launch).  The
// value is the same; only the instruction that computes it differs.
__device__ __forceinline__ float lone(float v) {
    asm volatile("" : "+v"(v));
    return v;
}

// one row of the two small nets: the four outputs m0 .. m0 + 3 of the WeightNet times rho.  cn: the packed constants in LDS.
__device__ __forceinline__ void small_nets(const float* cn, float dx, float dy, float dz, float dens, int m0, float (&rw)[4]) {
    float h1[8], h2[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const float* w = cn + WN_W1 + 3 * j;
        h1[j] = relu_bn(fmaf(w[2], dz, fmaf(w[1], dy, w[0] * dx)), cn[WN_S1 + j], cn[WN_T1 + j]);
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const float* w = cn + WN_W2 + 8 * j;
        float y = w[0] * h1[0];
#pragma unroll
        for (int k = 1; k < 8; ++k) y = fmaf(w[k], h1[k], y);
        h2[j] = relu_bn(y, cn[WN_S2 + j], cn[WN_T2 + j]);
    }
    float e1[8], e2[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) e1[j] = relu_bn(cn[DN_W1 + j] * dens, cn[DN_S1 + j], cn[DN_T1 + j]);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const float* w = cn + DN_W2 + 8 * j;
        float y = w[0] * e1[0];
#pragma unroll
        for (int k = 1; k < 8; ++k) y = fmaf(w[k], e1[k], y);
        e2[j] = relu_bn(y, cn[DN_S2 + j], cn[DN_T2 + j]);
    }
    float yr = cn[DN_W3] * e2[0];
#pragma unroll
    for (int k = 1; k < 8; ++k) yr = fmaf(cn[DN_W3 + k], e2[k], yr);
    const float rho = relu_bn(yr, cn[DN_S3], cn[DN_T3]);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const float* w = cn + WN_W3 + 8 * (m0 + i);
        float y = w[0] * h2[0];
#pragma unroll
        for (int k = 1; k < 8; ++k) y = fmaf(w[k], h2[k], y);
        rw[i] = rho * relu_bn(y, cn[WN_S3 + m0 + i], cn[WN_T3 + m0 + i]);
    }
}

template <int NS, int NL, int C1, int C2, int C3, bool BF16>
__global__ __launch_bounds__(NT, 2) void pointconv_level_infer_kernel(const PointConvArgs a) {
    using S = PointConvShape<NL, C1, C2, C3, BF16>;
    using XT = typename S::XT;
    constexpr int LD1 = S::LD1, LD2 = S::LD2, LDZ = S::LDZ;
    constexpr int NCB3 = C3 / 32, NJ3 = (NCB3 + 3) / 4;
    constexpr int GPT = RT / NS;                    // groups per tile
    constexpr int WPG = 4 / GPT;                    // waves per group in the contraction
    constexpr int NI = (C3 / 16) / WPG;             // 16-column blocks per wave
    static_assert(RT % NS == 0 && 4 % GPT == 0 && (C3 / 16) % WPG == 0 && NS % 4 == 0, "contraction split");
    extern __shared__ __attribute__((aligned(16))) float smem[];
    XT* X1 = reinterpret_cast<XT*>(smem);                                   // [RT][LD1]
    XT* X2 = X1 + RT * LD1;                                                 // [RT][LD2] (L = 3)
    float* Z = smem;                                                        // [RT][LDZ], over X1 | X2
    constexpr int KL = NL == 3 ? C2 : C1, LDL = NL == 3 ? LD2 : LD1;        // the last layer's input: X2, or X1 at L = 2
    const XT* XL = NL == 3 ? X2 : X1;
    float* RW = smem + S::tile_bytes / 4;                                   // [RT][16]
    float4* rloc = reinterpret_cast<float4*>(RW + RT * PC_M);               // [RT]
    int* rsrc = reinterpret_cast<int*>(rloc + RT);                          // [RT]
    float* rden = reinterpret_cast<float*>(rsrc + RT);                      // [RT]
    float* cn = rden + RT;                                                  // [PC_NETS]

    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, lr = lane & 31, lh = lane >> 5;
    const int g0 = blockIdx.x * a.GT;
    const int ngt = min(a.GT, a.G - g0);
    for (int e = tid; e < PC_NETS; e += NT) cn[e] = a.nets[e];
    // layer 1: a thread always works on the same four channels (NT is a multiple of C1 / 4): their constants in registers
    static_assert(NT % (C1 / 4) == 0, "layer-1 channel split");
    const int c4 = (tid % (C1 / 4)) * 4, r_first = tid / (C1 / 4);
    float wx[4][3], sc1[4], sh1[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int ch = c4 + i;
#pragma unroll
        for (int d = 0; d < 3; ++d) wx[i][d] = a.Wx[(size_t)ch * a.ldw + d];
        sc1[i] = a.sc1[ch]; sh1[i] = a.sh1[ch];
    }
    const int R = ngt * NS;

    for (int t0 = 0; t0 < R; t0 += RT) {
        const int nvalid = min(RT, R - t0);
        // 1. row records
        if (tid < RT) {
            const int rr = t0 + min(tid, nvalid - 1);
            const int gi = rr / NS, s = rr - gi * NS;
            const int g = g0 + gi, b = g / a.m;
            const int k = min(max(a.idx[(size_t)g * NS + s], 0), a.N - 1);
            const int src = b * a.N + k;
            const float* pk = a.xyz + (size_t)src * 3;
            const float* q = a.new_xyz + (size_t)g * 3;
            rloc[tid] = make_float4(__fsub_rn(pk[0], q[0]), __fsub_rn(pk[1], q[1]), __fsub_rn(pk[2], q[2]), 0.f);
            rsrc[tid] = src;
            rden[tid] = a.density[src];
        }
        __syncthreads();
        // 2. layer 1 (the folded first conv), four channels per thread; the small nets, four threads per row
        for (int r = r_first; r < RT; r += NT / (C1 / 4)) {
            const float4 L = rloc[r];
            float u[4] = {0.f, 0.f, 0.f, 0.f};
            if (a.Uf) {
                const float4 v = *reinterpret_cast<const float4*>(a.Uf + (size_t)rsrc[r] * C1 + c4);
                u[0] = v.x; u[1] = v.y; u[2] = v.z; u[3] = v.w;
            }
            float z[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                if constexpr (BF16) {              // the same chain, every step a single-lane instruction (lone(), above)
                    float y = lone(fmaf(wx[i][0], L.x, u[i]));
                    y = lone(fmaf(wx[i][1], L.y, y));
                    y = lone(fmaf(wx[i][2], L.z, y));
                    const float v = lone(lone(sc1[i] * y) + sh1[i]);
                    const float n = lone(v * a.slope);
                    z[i] = v > 0.f ? v : n;
                } else {
                    const float y = fmaf(wx[i][2], L.z, fmaf(wx[i][1], L.y, fmaf(wx[i][0], L.x, u[i])));
                    z[i] = act(sc1[i] * y + sh1[i], a.slope);
                }
            }
            tile_store4(X1 + (size_t)r * LD1 + c4, z);
        }
        {
            const int r = tid >> 2, m0 = (tid & 3) * 4;
            const float4 L = rloc[r];
            float rw[4];
            small_nets(cn, L.x, L.y, L.z, rden[r], m0, rw);
            *reinterpret_cast<float4*>(RW + r * PC_M + m0) = make_float4(rw[0], rw[1], rw[2], rw[3]);
        }
        __syncthreads();
        // 3. layer 2 (L = 3)
        if constexpr (NL == 3) {
            tile_layer<C1, LD1, C2, LD2>(X1, a.W2, a.sc2, a.sh2, a.slope, X2, wave, lane);
            __syncthreads();
        }
        // 4. the last layer -> Z (over X1 | X2: the barrier keeps the deposit behind every wave's last read of its input)
        {
            f32x16 acc[2][NJ3];
            if constexpr (BF16) mfma_layer_bf16<KL, LDL, NJ3, NCB3>(XL, reinterpret_cast<const __bf16*>(a.W3), wave, lane, acc);
            else mfma_layer<KL, LDL, NJ3, NCB3>(XL, a.W3, wave, lane, acc);
            __syncthreads();
#pragma unroll
            for (int j = 0; j < NJ3; ++j) {
                const int cb = wave + 4 * j;
                if (cb < NCB3) {
                    const int col = cb * 32 + lr;
                    const float sc = a.sc3[col], sh = a.sh3[col];
#pragma unroll
                    for (int rb = 0; rb < 2; ++rb)
#pragma unroll
                        for (int r = 0; r < 16; ++r) Z[acc_row(rb, r, lh) * LDZ + col] = act(sc * acc[rb][j][r] + sh, a.slope);
                }
            }
        }
        __syncthreads();
        // 5. the contraction of the tile's groups: wave -> (group of the tile, four 16-column blocks)
        {
            const int gt = wave / WPG;                               // group within the tile
            const int gi = t0 / NS + gt;                             // ... within the workgroup
            if (gi < ngt) {                                          // (uniform per wave)
                const int cb0 = (wave % WPG) * NI;
                const int kk = lane >> 4, j16 = lane & 15;
                const float* pa = RW + (gt * NS + kk) * PC_M + j16;
                const float* pb = Z + (gt * NS + kk) * LDZ + cb0 * 16 + j16;
                f32x4 acc[NI];
#pragma unroll
                for (int i = 0; i < NI; ++i) acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
                for (int q = 0; q < NS / 4; ++q) {
                    const float av = pa[4 * q * PC_M];
#pragma unroll
                    for (int i = 0; i < NI; ++i) acc[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, pb[4 * q * LDZ + 16 * i], acc[i], 0, 0, 0);
                }
                float* o = a.out + (size_t)(g0 + gi) * a.ldo + 4 * kk;
#pragma unroll
                for (int i = 0; i < NI; ++i) {
                    const int c = (cb0 + i) * 16 + j16;
                    *reinterpret_cast<float4*>(o + (size_t)c * PC_M) = make_float4(acc[i][0], acc[i][1], acc[i][2], acc[i][3]);
                }
            }
        }
        __syncthreads();
    }
}

// What every entry point of this argument list checks behind its own shape table, all before any HIP call, and the argument struct
// (GT is the launch's to set).  W3 / sc3 / sh3 are the last layer's whatever L is; W2 / sc2 / sh2 the middle layer's of L = 3.
// Uf, W[1], W[2] and out are moved in 16-byte pieces: their alignment is the caller's precondition (include/pcl_hip.h), held by
// pointcloudlib_amd/inference.py before the call; there is no other path to choose here.
inline int pointconv_args(const char* fn, const float* xyz, const float* new_xyz, const float* Uf, const float* Wx, int ldw,
                          const float* density, const int32_t* idx, int B, int N, int m, int L, const int32_t* widths,
                          const void* const* W, const float* const* scale, const float* const* shift, float slope, const float* nets,
                          int M, float* out, int ldo, PointConvArgs& a) {
    const int C3 = widths[L - 1];
    PCL_REQUIRE(xyz && new_xyz && Wx && density && idx && nets && out, "%s: null pointer", fn);
    PCL_REQUIRE(ldw >= 3, "%s: ldw=%d", fn, ldw);
    PCL_REQUIRE(B >= 1 && N >= 1 && m >= 1, "%s: bad sizes B=%d N=%d m=%d", fn, B, N, m);
    PCL_REQUIRE((size_t)B * m < (1u << 31) && (size_t)B * N < (1u << 31), "%s: too many groups / points", fn);
    for (int l = 0; l < L; ++l) PCL_REQUIRE(scale[l] && shift[l] && (l == 0 || W[l]), "%s: layer %d: null pointer", fn, l);
    PCL_REQUIRE(ldo >= C3 * M && ldo % 4 == 0, "%s: ldo=%d for %d columns (a multiple of 4)", fn, ldo, C3 * M);
    a = {};
    a.xyz = xyz; a.new_xyz = new_xyz; a.Uf = Uf; a.Wx = Wx; a.ldw = ldw; a.density = density; a.idx = idx;
    a.G = B * m; a.N = N; a.m = m;
    if (L == 3) { a.W2 = static_cast<const float*>(W[1]); a.sc2 = scale[1]; a.sh2 = shift[1]; }
    a.W3 = static_cast<const float*>(W[L - 1]);
    a.sc1 = scale[0]; a.sh1 = shift[0]; a.sc3 = scale[L - 1]; a.sh3 = shift[L - 1];
    a.slope = slope; a.nets = nets; a.out = out; a.ldo = ldo;
    return PCL_OK;
}

// groups per workgroup of a launch over G groups (infer_pointconv.hip): the same for every instantiation and both precisions
int pointconv_group_tile(int ns, int G);
// the five bf16 kernels of the part-seg shapes, by the shape id of infer_pointconv.hip (2 .. 6): infer_pointconv_seg_bf16.hip
int launch_pointconv_seg_bf16(int sid, const char* fn, const PointConvArgs& a, hipStream_t st);

template <int NS, int L, int C1, int C2, int C3, bool BF16>
int launch_pointconv(const char* fn, PointConvArgs a, hipStream_t st) {
    using S = PointConvShape<L, C1, C2, C3, BF16>;
    a.GT = pointconv_group_tile(NS, a.G);
    auto kern = pointconv_level_infer_kernel<NS, L, C1, C2, C3, BF16>;
    if (int rc = lds_opt_in(kern, S::lds_bytes, fn)) return rc;
    const int blocks = (a.G + a.GT - 1) / a.GT;
    hipLaunchKernelGGL(kern, dim3(blocks), dim3(NT), S::lds_bytes, st, a);
    return check_launch(fn);
}

}  // namespace pointconv
}  // namespace pcl
