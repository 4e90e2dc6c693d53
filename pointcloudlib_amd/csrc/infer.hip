// infer.hip -- one ball-query set-abstraction level in evaluation mode as ONE launch (networks/cls/pointnet2.py:33-62 under
// train_cls.py:92-124's eval()): the folded first layer, the two 1x1 convs that follow, eval BatchNorm + activation after
// each, and the max over the group.  Activations never leave LDS and registers.
//
// A workgroup (4 waves) owns GT consecutive groups and walks their DISTINCT rows (max(cnt,1) per group, the rows
// pcl_group_linear_f32 emits; ball-query padding repeats the first hit, so skipping it does not change the max) in tiles
// of 64 rows.  Per tile:
//   1. row records (source point, xyz - centre, inline features) into LDS; the tile's tail repeats its last row;
//   2. layer 1 elementwise: y1 = Wx (xyz - centre) + Uf[src] (+ Wf_small feat), z1 = act(scale1 y1 + shift1) -> X1 (LDS);
//   3. layer 2 on the fp32 MFMA (v_mfma_f32_32x32x2_f32): wave w owns the 32-column blocks w, w+4, ... of both 32-row
//      blocks; A from X1 (ds_read_b128), B straight from the weight matrix in L2 (one 16-byte load per lane per 4 k-steps);
//      epilogue z2 = act(scale2 y2 + shift2) -> X2 (LDS);
//   4. layer 3 the same from X2; z3 = act(scale3 y3 + shift3) in registers, then per group of the tile (consecutive rows)
//      a masked max over the lane's 32 rows and across the two lane halves, folded into the running per-group max (rmax,
//      LDS).  The wave owns its columns for every tile: no atomics.
// The k order inside a block of 8 is permuted (lane half h holds k = 8q + 4h + i at k-step 4q + i) identically for A and
// B, so each lane moves 16-byte pieces; the sum is the same set of products in a different order.
//
// The bf16 instantiation (pcl_sa_level_infer_bf16_f32) is the same kernel with layers 2 and 3 on v_mfma_f32_32x32x16_bf16.
// Its numerics:
//   - layer 1 is the fp32 expression above, unchanged (the same fmaf chain, act(scale1 y1 + shift1)); the result is rounded
//     to nearest even into a bf16 X1;
//   - layers 2 and 3 are bf16 x bf16 products accumulated in fp32, k-blocks of 16 in ascending order; the epilogue
//     act(scale y + shift) runs in fp32 as in the fp32 kernel; z2 is rounded to nearest even into a bf16 X2;
//   - z3 is never rounded: the max per group is taken in fp32 registers and the output is fp32;
//   - Uf stays fp32 (pcl_linear_fwd_rows_f32, stats-free); Wx, Wf_small, scale and shift stay fp32;
//   - a group's result depends only on its own rows: not on B, on the group's place in the launch or on GT;
//   - no atomics, run-to-run identical; rounding is the plain C++ conversion (v_cvt_pk_bf16_f32).
// X1 / X2 are [64][C + 8] bf16 (infer_mfma.h), half the bytes of the fp32 tiles.
//
// The tile sizes, the MFMA steps, the accumulator-to-row map (infer::acc_row) and the 4-channel tile store come from
// infer_mfma.h.  Layers 2 and 3 keep their epilogue loops here: layer 3's max per group is this kernel's alone, and layer 2
// through infer::tile_layer compiled to 6 % more instructions and 4-6 more registers in this kernel's tile loop.
#include <type_traits>

#include "common.h"
#include "infer_mfma.h"

namespace pcl {
namespace {

using namespace infer;

constexpr int IF_MAXGT = 16;     // groups per workgroup at most
constexpr size_t IF_LDS_CAP = 80 * 1024;     // two workgroups per CU

struct InferArgs {
    const float* xyz; const float* new_xyz; const float* Uf; const float* Wx; const float* fs; const float* Wfs;
    int CF, ldw;
    const int32_t* idx; const int32_t* cnt;
    int G, N, m, ns, GT;
    const float* W2; const float* W3;
    const float* sc1; const float* sh1; const float* sc2; const float* sh2; const float* sc3; const float* sh3;
    float slope;
    float* out; int ldo, col0;
};

template <int C1, int C2, int C3, bool BF16>
struct InferShape {
    using XT = std::conditional_t<BF16, __bf16, float>;                    // element of X1 / X2
    static constexpr int LD1 = C1 + row_pad<XT>, LD2 = C2 + row_pad<XT>;
    static size_t lds_bytes(int GT) {
        return sizeof(XT) * ((size_t)RT * LD1 + RT * LD2) + 4 * (size_t)GT * C3 + 32 * RT + 8 * RT + 4 * (IF_MAXGT + 4);
    }
};

template <int C1, int C2, int C3, bool BF16>
__global__ __launch_bounds__(NT, 2) void sa_level_infer_kernel(const InferArgs a) {
    using S = InferShape<C1, C2, C3, BF16>;
    using XT = typename S::XT;
    constexpr int LD1 = S::LD1, LD2 = S::LD2;
    constexpr int NCB2 = C2 / 32, NCB3 = C3 / 32;
    constexpr int NJ2 = (NCB2 + 3) / 4, NJ3 = (NCB3 + 3) / 4;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int GT = a.GT;
    XT* X1 = reinterpret_cast<XT*>(smem);                   // [RT][LD1]
    XT* X2 = X1 + RT * LD1;                                 // [RT][LD2]
    float* rmax = reinterpret_cast<float*>(X2 + RT * LD2);                // [GT][C3]
    float4* rloc = reinterpret_cast<float4*>(rmax + (size_t)GT * C3);     // [RT]
    float4* rfeat = rloc + RT;                              // [RT]
    int* rsrc = reinterpret_cast<int*>(rfeat + RT);         // [RT]
    int* rgrp = rsrc + RT;                                  // [RT]
    int* gstart = rgrp + RT;                                // [GT + 1]

    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, lr = lane & 31, lh = lane >> 5;
    const int g0 = blockIdx.x * GT;
    const int ngt = min(GT, a.G - g0);
    if (tid == 0) {
        int run = 0;
        for (int i = 0; i < ngt; ++i) {
            gstart[i] = run;
            run += min(max(a.cnt[g0 + i], 1), a.ns);
        }
        gstart[ngt] = run;
    }
    for (int e = tid; e < ngt * C3; e += NT) rmax[e] = -INFINITY;
    // layer 1: a thread always works on the same four channels (NT is a multiple of C1 / 4): their constants in registers
    static_assert(NT % (C1 / 4) == 0, "layer-1 channel split");
    const int c4 = (tid % (C1 / 4)) * 4, r_first = tid / (C1 / 4);
    float wx[4][3], wf[4][4], sc1[4], sh1[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int ch = c4 + i;
#pragma unroll
        for (int d = 0; d < 3; ++d) wx[i][d] = a.Wx ? a.Wx[(size_t)ch * a.ldw + d] : 0.f;
#pragma unroll
        for (int f = 0; f < 4; ++f) wf[i][f] = f < a.CF ? a.Wfs[(size_t)ch * a.ldw + f] : 0.f;
        sc1[i] = a.sc1[ch]; sh1[i] = a.sh1[ch];
    }
    __syncthreads();
    const int R = gstart[ngt];

    for (int t0 = 0; t0 < R; t0 += RT) {
        const int nvalid = min(RT, R - t0);
        // 1. row records
        if (tid < RT) {
            const int rr = t0 + min(tid, nvalid - 1);
            int gi = 0;
            while (gi + 1 < ngt && gstart[gi + 1] <= rr) ++gi;
            const int g = g0 + gi, s = rr - gstart[gi], b = g / a.m;
            const int k = min(max(a.idx[(size_t)g * a.ns + s], 0), a.N - 1);
            const int src = b * a.N + k;
            rsrc[tid] = src;
            rgrp[tid] = gi;
            float4 L = make_float4(0.f, 0.f, 0.f, 0.f);
            if (a.Wx) {
                const float* pk = a.xyz + (size_t)src * 3;
                const float* q = a.new_xyz + (size_t)g * 3;
                L.x = __fsub_rn(pk[0], q[0]); L.y = __fsub_rn(pk[1], q[1]); L.z = __fsub_rn(pk[2], q[2]);
            }
            rloc[tid] = L;
            float f[4] = {0.f, 0.f, 0.f, 0.f};
            for (int j = 0; j < a.CF; ++j) f[j] = a.fs[(size_t)src * a.CF + j];
            rfeat[tid] = make_float4(f[0], f[1], f[2], f[3]);
        }
        __syncthreads();
        // 2. layer 1 (the folded first conv), four channels per thread
        for (int r = r_first; r < RT; r += NT / (C1 / 4)) {
            const float4 L = rloc[r], F = rfeat[r];
            float u[4] = {0.f, 0.f, 0.f, 0.f};
            if (a.Uf) {
                const float4 v = *reinterpret_cast<const float4*>(a.Uf + (size_t)rsrc[r] * C1 + c4);
                u[0] = v.x; u[1] = v.y; u[2] = v.z; u[3] = v.w;
            }
            float z[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                float y = fmaf(wx[i][2], L.z, fmaf(wx[i][1], L.y, fmaf(wx[i][0], L.x, u[i])));
                y = fmaf(wf[i][3], F.w, fmaf(wf[i][2], F.z, fmaf(wf[i][1], F.y, fmaf(wf[i][0], F.x, y))));
                z[i] = act(sc1[i] * y + sh1[i], a.slope);
            }
            tile_store4(X1 + (size_t)r * LD1 + c4, z);
        }
        __syncthreads();
        // 3. layer 2
        {
            f32x16 acc[2][NJ2];
            if constexpr (BF16) mfma_layer_bf16<C1, LD1, NJ2, NCB2>(X1, reinterpret_cast<const __bf16*>(a.W2), wave, lane, acc);
            else mfma_layer<C1, LD1, NJ2, NCB2>(X1, a.W2, wave, lane, acc);
#pragma unroll
            for (int j = 0; j < NJ2; ++j) {
                const int cb = wave + 4 * j;
                if (cb < NCB2) {
                    const int col = cb * 32 + lr;
                    const float sc = a.sc2[col], sh = a.sh2[col];
#pragma unroll
                    for (int rb = 0; rb < 2; ++rb)
#pragma unroll
                        for (int r = 0; r < 16; ++r) {
                            const int row = acc_row(rb, r, lh);
                            X2[(size_t)row * LD2 + col] = (XT)act(sc * acc[rb][j][r] + sh, a.slope);
                        }
                }
            }
        }
        __syncthreads();
        // 4. layer 3 + running max per group
        {
            f32x16 acc[2][NJ3];
            if constexpr (BF16) mfma_layer_bf16<C2, LD2, NJ3, NCB3>(X2, reinterpret_cast<const __bf16*>(a.W3), wave, lane, acc);
            else mfma_layer<C2, LD2, NJ3, NCB3>(X2, a.W3, wave, lane, acc);
            // the groups of this tile occupy consecutive row ranges: one masked max per group over the lane's 32 rows, then
            // across the two lane halves (same column, interleaved rows)
            const int glo = rgrp[0], ghi = rgrp[nvalid - 1];
#pragma unroll
            for (int j = 0; j < NJ3; ++j) {
                const int cb = wave + 4 * j;
                if (cb < NCB3) {
                    const int col = cb * 32 + lr;
                    const float sc = a.sc3[col], sh = a.sh3[col];
#pragma unroll
                    for (int rb = 0; rb < 2; ++rb)
#pragma unroll
                        for (int r = 0; r < 16; ++r) acc[rb][j][r] = act(sc * acc[rb][j][r] + sh, a.slope);
                    for (int gi = glo; gi <= ghi; ++gi) {
                        const int lo = gstart[gi] - t0, hi = min(gstart[gi + 1] - t0, nvalid);
                        float mx = -INFINITY;
#pragma unroll
                        for (int rb = 0; rb < 2; ++rb)
#pragma unroll
                            for (int r = 0; r < 16; ++r) {
                                const int row = acc_row(rb, r, lh);
                                if (row >= lo && row < hi) mx = fmaxf(mx, acc[rb][j][r]);
                            }
                        mx = fmaxf(mx, __shfl_xor(mx, 32));
                        if (lh == 0) rmax[gi * C3 + col] = fmaxf(rmax[gi * C3 + col], mx);
                    }
                }
            }
        }
        __syncthreads();
    }
    for (int e = tid; e < ngt * C3; e += NT) {
        const int gi = e / C3, c = e - gi * C3;
        a.out[(size_t)(g0 + gi) * a.ldo + a.col0 + c] = rmax[e];
    }
}

template <int C1, int C2, int C3, bool BF16>
int launch_infer(const char* fn, InferArgs a, hipStream_t st) {
    using S = InferShape<C1, C2, C3, BF16>;
    int GT = min(IF_MAXGT, max(1, 512 / a.ns));
    while (GT > 1 && S::lds_bytes(GT) > IF_LDS_CAP) --GT;
    a.GT = GT;
    const size_t lds = S::lds_bytes(GT);
    auto kern = sa_level_infer_kernel<C1, C2, C3, BF16>;
    if (int rc = lds_opt_in(kern, lds, fn)) return rc;
    const int blocks = (a.G + GT - 1) / GT;
    hipLaunchKernelGGL(kern, dim3(blocks), dim3(NT), lds, st, a);
    return check_launch(fn);
}

// the widths after the fold that have a kernel: the SA levels of networks/cls/pointnet2.py (SSG and MSG)
int infer_shape_id(int L, const int* w) {
    if (L != 3) return -1;
    if (w[0] == 32 && w[1] == 32 && w[2] == 64) return 0;
    if (w[0] == 64 && w[1] == 64 && w[2] == 128) return 1;
    if (w[0] == 64 && w[1] == 96 && w[2] == 128) return 2;
    if (w[0] == 128 && w[1] == 128 && w[2] == 256) return 3;
    return -1;
}

constexpr int IF_MAXNS = 1024;

}  // namespace
}  // namespace pcl
using namespace pcl;

extern "C" int pcl_sa_level_infer_supported(int ns, int L, int C1, int C2, int C3, int C4) {
    const int w[4] = {C1, C2, C3, C4};
    return ns >= 1 && ns <= IF_MAXNS && L >= 1 && L <= 4 && infer_shape_id(L, w) >= 0;
}

namespace pcl {
namespace {

// both precisions: every check runs before any HIP call.  W[l], l >= 1: fp32 (BF16 false) or bf16 (true) [C_l][C_{l-1}]
template <bool BF16>
int sa_level_infer(const char* fn, const float* xyz, const float* new_xyz, const float* Uf, const float* Wx, const float* feat_small,
                   const float* Wf_small, int CF, int ldw, const int32_t* idx, const int32_t* cnt, int B, int N, int m, int ns, int L,
                   const int32_t* widths, const void* const* W, const float* const* scale, const float* const* shift, float slope,
                   float* out, int ldo, int col0, void* stream) {
    PCL_REQUIRE(widths && W && scale && shift, "%s: null host array", fn);
    PCL_REQUIRE(L >= 1 && L <= 4, "%s: L=%d", fn, L);
    const int sid = infer_shape_id(L, widths);
    PCL_REQUIRE(sid >= 0 && ns >= 1 && ns <= IF_MAXNS,
                "%s: no kernel for ns=%d L=%d widths %d/%d/%d (pcl_sa_level_infer_supported)", fn, ns, L, widths[0],
                L > 1 ? widths[1] : 0, L > 2 ? widths[2] : 0);
    PCL_REQUIRE(idx && cnt && out, "%s: null pointer", fn);
    PCL_REQUIRE(Uf || Wx || CF > 0, "%s: need features (Uf or feat_small) and/or coordinates (Wx)", fn);
    PCL_REQUIRE(CF >= 0 && CF <= 4 && (CF == 0 || (feat_small && Wf_small)), "%s: CF=%d inline features (<= 4)", fn, CF);
    PCL_REQUIRE(!Wx || (xyz && new_xyz), "%s: Wx needs xyz and new_xyz", fn);
    PCL_REQUIRE(ldw >= (Wx ? 3 : 0) && ldw >= CF, "%s: ldw=%d", fn, ldw);
    PCL_REQUIRE(B >= 1 && N >= 1 && m >= 1, "%s: bad sizes B=%d N=%d m=%d", fn, B, N, m);
    PCL_REQUIRE((size_t)B * m < (1u << 31) && (size_t)B * N < (1u << 31), "%s: too many groups / points", fn);
    for (int l = 0; l < L; ++l) PCL_REQUIRE(scale[l] && shift[l] && (l == 0 || W[l]), "%s: layer %d: null pointer", fn, l);
    const int CL = widths[L - 1];
    PCL_REQUIRE(col0 >= 0 && ldo >= col0 + CL, "%s: ldo=%d col0=%d for %d channels", fn, ldo, col0, CL);
    bool aligned = al16(Uf);
    for (int l = 1; l < L; ++l) aligned = aligned && al16(W[l]);
    PCL_REQUIRE(aligned, "%s: Uf and the weights must be 16-byte aligned", fn);
    InferArgs a = {};
    a.xyz = xyz; a.new_xyz = new_xyz; a.Uf = Uf; a.Wx = Wx; a.fs = feat_small; a.Wfs = Wf_small; a.CF = CF; a.ldw = ldw;
    a.idx = idx; a.cnt = cnt; a.G = B * m; a.N = N; a.m = m; a.ns = ns;
    a.W2 = static_cast<const float*>(W[1]); a.W3 = static_cast<const float*>(W[2]);
    a.sc1 = scale[0]; a.sh1 = shift[0]; a.sc2 = scale[1]; a.sh2 = shift[1]; a.sc3 = scale[2]; a.sh3 = shift[2];
    a.slope = slope; a.out = out; a.ldo = ldo; a.col0 = col0;
    hipStream_t st = as_stream(stream);
    switch (sid) {
        case 0: return launch_infer<32, 32, 64, BF16>(fn, a, st);
        case 1: return launch_infer<64, 64, 128, BF16>(fn, a, st);
        case 2: return launch_infer<64, 96, 128, BF16>(fn, a, st);
        default: return launch_infer<128, 128, 256, BF16>(fn, a, st);
    }
}

}  // namespace
}  // namespace pcl

extern "C" int pcl_sa_level_infer_f32(const float* xyz, const float* new_xyz, const float* Uf, const float* Wx, const float* feat_small,
                                      const float* Wf_small, int CF, int ldw, const int32_t* idx, const int32_t* cnt, int B, int N, int m,
                                      int ns, int L, const int32_t* widths, const float* const* W, const float* const* scale,
                                      const float* const* shift, float slope, float* out, int ldo, int col0, void* stream) {
    return sa_level_infer<false>("pcl_sa_level_infer_f32", xyz, new_xyz, Uf, Wx, feat_small, Wf_small, CF, ldw, idx, cnt, B, N, m, ns, L,
                                 widths, reinterpret_cast<const void* const*>(W), scale, shift, slope, out, ldo, col0, stream);
}

extern "C" int pcl_sa_level_infer_bf16_f32(const float* xyz, const float* new_xyz, const float* Uf, const float* Wx, const float* feat_small,
                                           const float* Wf_small, int CF, int ldw, const int32_t* idx, const int32_t* cnt, int B, int N,
                                           int m, int ns, int L, const int32_t* widths, const void* const* W, const float* const* scale,
                                           const float* const* shift, float slope, float* out, int ldo, int col0, void* stream) {
    return sa_level_infer<true>("pcl_sa_level_infer_bf16_f32", xyz, new_xyz, Uf, Wx, feat_small, Wf_small, CF, ldw, idx, cnt, B, N, m, ns,
                                L, widths, W, scale, shift, slope, out, ldo, col0, stream);
}
