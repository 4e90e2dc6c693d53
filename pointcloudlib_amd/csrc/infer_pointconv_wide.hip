// infer_pointconv_wide.hip -- the fused k-NN PointConv level (infer_pointconv.h) for the two 512-wide levels of
// networks/seg/pointconv_partseg.py, whose last activation Z [64][512 + 16] fp32 (135 168 B) does not fit that kernel's tile:
//     sa3: 32 neighbours, 256/256/512        in0: 16 neighbours, 512/512 (two layers)
// pcl_pointconv_wide_level_infer_f32, its shape table and group tile; fp32 only.  It computes what infer_pointconv.h's kernel
// computes, value by value: the row records, the folded layer 1 (+ Uf), the two small nets and rw, the middle layer (sa3), the
// last layer with eval BatchNorm and activation, and out[g, c*16 + m] = sum_s z[s, c] rho[s] w[s, m] on v_mfma_f32_16x16x4_f32
// with s ascending -- steps 1 to 3 are that kernel's text, on its pieces (small_nets, tile_layer, mfma_layer, acc_row, tile_store4,
// act).
//
// What differs: Z never exists at full width.  The last layer and the contraction run in chunks of CH columns (steps 4 and 5 of
// infer_pointconv.h inside one loop): the chunk's weight rows are W_last + c0 * K, scale, shift and the output columns are offset
// by c0, and the chunk's activations are deposited in Z [64][CH + 16] and contracted from there.  A column of the last layer is
// the whole k chain of mfma_layer and a column of the output the whole s chain of the contraction, so every output is the same
// chain of operations whatever CH is.
//
// One workgroup (4 waves) per compute unit, __launch_bounds__(NT, 1), on up to 160 KiB of dynamic LDS (WideShape):
//   sa3: X1 | X2 [64][260] each (133 120 B); Z [64][144] (CH = 128, 36 864 B) lies over X1, which is dead once layer 2 has run
//        (the barrier behind tile_layer); RW, row records and constants 7 232 B: 140 352 B.
//   in0: X1 [64][516] (132 096 B) is the last layer's input and is read by every chunk, so Z [64][80] (CH = 64, 20 480 B) lies
//        behind it: 159 808 B.  A chunk is two 32-column blocks: the four waves split it by row block as well (mfma_block with one
//        row block; mfma_layer would leave waves 2 and 3 without a block).
// The last layer runs on mfma_block (below): mfma_layer's products in mfma_layer's order, with four weight pieces in flight
// (three k-blocks ahead), because nothing else hides a load here -- one wave per SIMD.  The first build ran the last layer on mfma_layer
// itself and measured 0.626 / 0.794 ms per launch (sa3 / in0, B = 64, N = 2048) against 0.509 / 0.379 ms for this one, and sa3
// 0.328 ms with the group tile below.
// Z's row strides 144 and 80 are 16 (mod 32) floats, the pattern of infer_pointconv.h's LDZ: no bank conflicts in the deposit or in
// the contraction's reads.
// Barriers: Z is never over the input of the layer that fills it, so a chunk is MFMA -> deposit -> barrier -> contraction ->
// barrier; the second one keeps the next chunk's deposit (and, behind the last chunk, the next tile's layer 1 and row records)
// behind every wave's reads.  Every barrier is outside wave-divergent branches.  In the contraction a wave owns four 16-column
// blocks of one group of the tile at either shape (ns = 32: two groups, two waves each, CH / 16 = 8 blocks; ns = 16: four groups,
// one wave each, 4 blocks).
//
// Numeric contract (include/pcl_hip.h): a group's result depends only on its own rows (not on B, on the group's place in the
// launch, on GT or on CH); no atomics, two calls give identical bits; out is fully defined for every group; idx is clamped to
// [0, N - 1].
#include "infer_pointconv.h"

namespace pcl {
namespace pointconv {

constexpr size_t PCW_LDS_CAP = 160 * 1024;         // one workgroup per CU: all of a compute unit's LDS

// CH: columns of the last layer per chunk
template <int NS, int L, int C1, int C2, int C3, int CH>
struct WideShape {
    static_assert(L == 2 || L == 3, "layers of the feature MLP");
    static_assert(C3 % CH == 0 && CH % 32 == 0 && (CH + 16) % 32 == 16, "chunks of whole 32-column blocks; Z's row stride");
    static constexpr int LD1 = C1 + row_pad<float>, LD2 = C2 + row_pad<float>, LDZ = CH + 16;
    static constexpr size_t x1_bytes = 4 * (size_t)RT * LD1, x2_bytes = L == 3 ? 4 * (size_t)RT * LD2 : 0, z_bytes = 4 * (size_t)RT * LDZ;
    // L = 3: Z over X1 (dead after layer 2); L = 2: Z behind X1 (the last layer's input)
    static_assert(L == 2 || z_bytes <= x1_bytes, "Z lies over X1");
    static constexpr size_t z_off = L == 3 ? 0 : x1_bytes;
    static constexpr size_t tile_bytes = x1_bytes + x2_bytes + (L == 3 ? 0 : z_bytes);
    // RW, row records (d, src, density), the small nets' constants: as PointConvShape
    static constexpr size_t lds_bytes = tile_bytes + 4 * (size_t)RT * PC_M + 16 * RT + 4 * RT + 4 * RT + 4 * PC_NETS;
    static_assert(lds_bytes <= PCW_LDS_CAP, "one workgroup per CU");
};

constexpr int PCW_PF = 4;                          // weight pieces a lane keeps in flight in mfma_block

// ONE 32-column block of a layer for NRB 32-row blocks: acc[rb] = X[rb*32 + row][k] * W[col][k] over k < K (X in LDS at the first
// of the row blocks, row stride LDX; W [32][K] in global memory at the column block's first row).  The products and their order
// are mfma_layer's (k-blocks of 8 ascending, the permutation of infer_mfma.h inside a block), so an element is the same fp32
// chain as there.  What differs is for a workgroup that is alone on its compute unit, with no second wave on the SIMD to hide a
// weight load behind: PCW_PF of the lane's 16-byte weight pieces are in flight, PCW_PF - 1 k-blocks ahead (mfma_layer: one), the
// tile's pieces are read one k-block ahead, and NRB = 1 lets the four waves split a chunk of two column blocks by rows, where
// mfma_layer would leave two of them without a block.
template <int K, int LDX, int NRB>
__device__ __forceinline__ void mfma_block(const float* __restrict__ X, const float* __restrict__ W, int lane, f32x16 (&acc)[NRB]) {
    static_assert((K / 8) % PCW_PF == 0 && K / 8 >= PCW_PF, "k-blocks in whole rounds of the pieces in flight");
    const int lr = lane & 31, lh = lane >> 5;
    const float* xa = X + (size_t)lr * LDX + 4 * lh;
    const float* wb = W + (size_t)lr * K + 4 * lh;
#pragma unroll
    for (int rb = 0; rb < NRB; ++rb)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[rb][r] = 0.f;
    float4 b[PCW_PF];
#pragma unroll
    for (int i = 0; i < PCW_PF; ++i) b[i] = *reinterpret_cast<const float4*>(wb + 8 * i);
    float4 av[2][NRB];                                                     // the tile's pieces of this k-block and of the next
#pragma unroll
    for (int rb = 0; rb < NRB; ++rb) av[0][rb] = *reinterpret_cast<const float4*>(xa + (size_t)rb * 32 * LDX);
    // A round is PCW_PF k-blocks.  It stays a loop, the last round (which loads no weights) apart from it, and the order inside a
    // step is pinned (sched_barrier): the tile's pieces of the next k-block, this k-block's MFMAs, then the weight piece that takes
    // the place of the one just used -- so no value is copied from register to register (a copy of a loaded value waits for the
    // load).  Unrolled and left to the scheduler, the weight loads came out one k-block ahead of their use and the tile's pieces
    // right in front of it, and every step waited for both.
    auto round = [&](int q0, auto more) {
#pragma unroll
        for (int i = 0; i < PCW_PF; ++i) {
            static_assert(PCW_PF % 2 == 0, "the two buffers of the tile's pieces alternate by step");
            if (more.value || i + 1 < PCW_PF) {
#pragma unroll
                for (int rb = 0; rb < NRB; ++rb)
                    av[(i + 1) & 1][rb] = *reinterpret_cast<const float4*>(xa + (size_t)rb * 32 * LDX + 8 * (q0 + i + 1));
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int rb = 0; rb < NRB; ++rb) acc[rb] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[i & 1][rb].x, b[i].x, acc[rb], 0, 0, 0);
#pragma unroll
            for (int rb = 0; rb < NRB; ++rb) acc[rb] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[i & 1][rb].y, b[i].y, acc[rb], 0, 0, 0);
#pragma unroll
            for (int rb = 0; rb < NRB; ++rb) acc[rb] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[i & 1][rb].z, b[i].z, acc[rb], 0, 0, 0);
#pragma unroll
            for (int rb = 0; rb < NRB; ++rb) acc[rb] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[i & 1][rb].w, b[i].w, acc[rb], 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
            if constexpr (more.value) b[i] = *reinterpret_cast<const float4*>(wb + 8 * (q0 + PCW_PF + i));
        }
    };
#pragma unroll 1
    for (int q0 = 0; q0 < K / 8 - PCW_PF; q0 += PCW_PF) round(q0, std::true_type{});
    round(K / 8 - PCW_PF, std::false_type{});
}

template <int NS, int NL, int C1, int C2, int C3, int CH>
__global__ __launch_bounds__(NT, 1) void pointconv_wide_level_infer_kernel(const PointConvArgs a) {
    using S = WideShape<NS, NL, C1, C2, C3, CH>;
    constexpr int LD1 = S::LD1, LD2 = S::LD2, LDZ = S::LDZ;
    // the last layer: a chunk is four (32-row block, 32-column block) pairs per pass of the four waves -- four column blocks of
    // both row blocks each (CH = 128), or two column blocks split by row block (CH = 64)
    constexpr int NCB = CH / 32, NRB = NCB / 2;
    static_assert(NCB == 4 || NCB == 2, "one column block per wave, or two waves per column block");
    constexpr int GPT = RT / NS;                    // groups per tile
    constexpr int WPG = 4 / GPT;                    // waves per group in the contraction
    constexpr int NI = (CH / 16) / WPG;             // 16-column blocks per wave and chunk
    static_assert(RT % NS == 0 && 4 % GPT == 0 && (CH / 16) % WPG == 0 && NS % 4 == 0, "contraction split");
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* X1 = smem;                                                       // [RT][LD1]
    float* X2 = X1 + RT * LD1;                                              // [RT][LD2] (L = 3)
    float* Z = smem + S::z_off / 4;                                         // [RT][LDZ]: one chunk of the last activation
    constexpr int KL = NL == 3 ? C2 : C1, LDL = NL == 3 ? LD2 : LD1;        // the last layer's input: X2, or X1 at L = 2
    const float* XL = NL == 3 ? X2 : X1;
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
                const float y = fmaf(wx[i][2], L.z, fmaf(wx[i][1], L.y, fmaf(wx[i][0], L.x, u[i])));
                z[i] = act(sc1[i] * y + sh1[i], a.slope);
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
        // 3. layer 2 (L = 3); behind its barrier X1 is dead and Z may lie over it
        if constexpr (NL == 3) {
            tile_layer<C1, LD1, C2, LD2>(X1, a.W2, a.sc2, a.sh2, a.slope, X2, wave, lane);
            __syncthreads();
        }
        // 4. + 5. the last layer and the contraction, CH columns at a time
        const int gt = wave / WPG;                                   // the wave's group within the tile
        const int gi = t0 / NS + gt;                                 // ... within the workgroup
        const int cb0 = (wave % WPG) * NI;                           // its first 16-column block of a chunk
        const int kk = lane >> 4, j16 = lane & 15;
        const int cbw = NCB == 4 ? wave : (wave & 1), rb0 = NCB == 4 ? 0 : (wave >> 1);   // the wave's block(s) of the last layer
#pragma unroll 1
        for (int c0 = 0; c0 < C3; c0 += CH) {
            {
                f32x16 acc[NRB];
                mfma_block<KL, LDL, NRB>(XL + (size_t)rb0 * 32 * LDL, a.W3 + (size_t)(c0 + cbw * 32) * KL, lane, acc);
                const int col = cbw * 32 + lr;
                const float sc = a.sc3[c0 + col], sh = a.sh3[c0 + col];
#pragma unroll
                for (int rb = 0; rb < NRB; ++rb)
#pragma unroll
                    for (int r = 0; r < 16; ++r) Z[acc_row(rb0 + rb, r, lh) * LDZ + col] = act(sc * acc[rb][r] + sh, a.slope);
            }
            __syncthreads();
            if (gi < ngt) {                                          // (uniform per wave)
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
                    const int c = c0 + (cb0 + i) * 16 + j16;
                    *reinterpret_cast<float4*>(o + (size_t)c * PC_M) = make_float4(acc[i][0], acc[i][1], acc[i][2], acc[i][3]);
                }
            }
            __syncthreads();
        }
    }
}

// groups per workgroup: whole tiles, 1 .. PC_MAXTILES of them.  One workgroup runs per compute unit, so a launch takes
// ceil(workgroups / CUs) rounds of `tiles` tiles each: the count with the fewest tile times wins, the larger of equal ones (fewer
// workgroups load the constants).  Halving from PC_MAXTILES as pointconv_group_tile does gave sa3 at B = 64 (1152 tiles) 288
// workgroups of 4 tiles on 256 compute units -- two rounds, the second with 32 workgroups, 8 tile times where 5 suffice.
int pointconv_wide_group_tile(int ns, int G) {
    const int gpt = RT / ns, cus = cu_count();
    const long long T = ((long long)G + gpt - 1) / gpt;
    int best = 1;
    long long best_time = -1;
    for (int tiles = 1; tiles <= PC_MAXTILES; ++tiles) {
        const long long wgs = (T + tiles - 1) / tiles, time = (wgs + cus - 1) / cus * tiles;
        if (best_time < 0 || time <= best_time) { best = tiles; best_time = time; }
    }
    return best * gpt;
}

template <int NS, int L, int C1, int C2, int C3, int CH>
int launch_pointconv_wide(const char* fn, PointConvArgs a, hipStream_t st) {
    using S = WideShape<NS, L, C1, C2, C3, CH>;
    a.GT = pointconv_wide_group_tile(NS, a.G);
    auto kern = pointconv_wide_level_infer_kernel<NS, L, C1, C2, C3, CH>;
    if (int rc = lds_opt_in(kern, S::lds_bytes, fn)) return rc;
    const int blocks = (a.G + a.GT - 1) / a.GT;
    hipLaunchKernelGGL(kern, dim3(blocks), dim3(NT), S::lds_bytes, st, a);
    return check_launch(fn);
}

// sa3 and in0 of networks/seg/pointconv_partseg.py (C2 = widths[1], C3 = widths[L-1]: C2 = C3 at L = 2)
int pointconv_wide_shape_id(int ns, int L, int C1, int C2, int C3, int M) {
    if (M != PC_M) return -1;
    if (L == 3 && ns == 32 && C1 == 256 && C2 == 256 && C3 == 512) return 0;
    if (L == 2 && ns == 16 && C1 == 512 && C2 == 512 && C3 == 512) return 1;
    return -1;
}

}  // namespace pointconv
}  // namespace pcl
using namespace pcl;
using namespace pcl::pointconv;

extern "C" int pcl_pointconv_wide_level_infer_supported(int ns, int L, int C1, int C2, int C3, int M) {
    return pointconv_wide_shape_id(ns, L, C1, C2, C3, M) >= 0;
}

extern "C" int pcl_pointconv_wide_level_infer_group_tile(int ns, int G) {
    return (ns == 16 || ns == 32) && G >= 1 ? pointconv_wide_group_tile(ns, G) : 0;
}

extern "C" int pcl_pointconv_wide_level_infer_f32(const float* xyz, const float* new_xyz, const float* Uf, const float* Wx, int ldw,
                                                  const float* density, const int32_t* idx, int B, int N, int m, int ns, int L,
                                                  const int32_t* widths, const float* const* W, const float* const* scale,
                                                  const float* const* shift, float slope, const float* nets, int M, float* out, int ldo,
                                                  void* stream) {
    const char* fn = "pcl_pointconv_wide_level_infer_f32";
    PCL_REQUIRE(widths && W && scale && shift, "%s: null host array", fn);
    PCL_REQUIRE(L >= 1 && L <= 4, "%s: L=%d", fn, L);
    const int sid = L == 2 || L == 3 ? pointconv_wide_shape_id(ns, L, widths[0], widths[1], widths[L - 1], M) : -1;
    PCL_REQUIRE(sid >= 0, "%s: no kernel for ns=%d L=%d widths %d/%d/%d M=%d (pcl_pointconv_wide_level_infer_supported)", fn, ns, L,
                widths[0], L > 1 ? widths[1] : 0, L > 2 ? widths[2] : 0, M);
    PointConvArgs a;
    if (int rc = pointconv_args(fn, xyz, new_xyz, Uf, Wx, ldw, density, idx, B, N, m, L, widths, reinterpret_cast<const void* const*>(W),
                                scale, shift, slope, nets, M, out, ldo, a))
        return rc;
    hipStream_t st = as_stream(stream);
    if (sid == 0) return launch_pointconv_wide<32, 3, 256, 256, 512, 128>(fn, a, st);
    return launch_pointconv_wide<16, 2, 512, 512, 512, 64>(fn, a, st);
}
