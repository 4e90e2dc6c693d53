// infer_pointconv.hip -- the entry points of the fused k-NN PointConv level (infer_pointconv.h has the kernel and its description):
// the shape tables, the host checks and the launches.  This file instantiates the seven fp32 kernels and the two bf16 kernels of
// pcl_pointconv_level_infer_bf16_f32; the five bf16 kernels of the part-seg shapes are instantiated in infer_pointconv_seg_bf16.hip
// (its header says why they are not instantiated here).  The two 512-wide levels of the part-seg network have another kernel and
// entry points of their own: infer_pointconv_wide.hip.
#include "infer_pointconv.h"

namespace pcl {
namespace pointconv {

// groups per workgroup: whole tiles, PC_MAXTILES of them, halved while the launch would have fewer than two workgroups per compute unit
int pointconv_group_tile(int ns, int G) {
    const int gpt = RT / ns;
    int tiles = PC_MAXTILES;
    const int want = 2 * cu_count();
    while (tiles > 1 && (G + tiles * gpt - 1) / (tiles * gpt) < want) tiles /= 2;
    return tiles * gpt;
}

}  // namespace pointconv
namespace {

using namespace infer;
using namespace pointconv;

// the (ns, widths) that have a kernel: sa1 and sa2 of networks/cls/pointconv.py
int pointconv_shape_id(int ns, int L, int C1, int C2, int C3, int M) {
    if (L != 3 || M != PC_M) return -1;
    if (ns == 32 && C1 == 64 && C2 == 64 && C3 == 128) return 0;
    if (ns == 64 && C1 == 128 && C2 == 128 && C3 == 256) return 1;
    return -1;
}

// every instantiation (pcl_pointconv_seg_level_infer_f32 and, with bf16 tiles, pcl_pointconv_seg_level_infer_bf16_f32): the two
// above keep their ids, then the levels of networks/seg/pointconv_partseg.py that fit the tile -- sa0, sa2 at ns = 32; in1, in2
// (two layers: C2 = C3 = widths[1]) and in3 at ns = 16.  sa3 (256/256/512) and in0 (512/512) need about 133 KB of LDS in this form
// (Z is fp32 under either element type) and are not in this table: their kernel is infer_pointconv_wide.hip's, which holds Z a
// column chunk at a time (pcl_pointconv_wide_level_infer_f32, a table of its own).
int pointconv_seg_shape_id(int ns, int L, int C1, int C2, int C3, int M) {
    const int sid = pointconv_shape_id(ns, L, C1, C2, C3, M);
    if (sid >= 0 || M != PC_M) return sid;
    if (L == 3 && ns == 32 && C1 == 32 && C2 == 32 && C3 == 64) return 2;
    if (L == 3 && ns == 32 && C1 == 128 && C2 == 128 && C3 == 256) return 3;
    if (L == 2 && ns == 16 && C1 == 256 && C2 == 256 && C3 == 256) return 4;
    if (L == 2 && ns == 16 && C1 == 128 && C2 == 128 && C3 == 128) return 5;
    if (L == 3 && ns == 16 && C1 == 128 && C2 == 128 && C3 == 128) return 6;
    return -1;
}

// both precisions and both shape tables (SEG: pointconv_seg_shape_id): every check runs before any HIP call.  W[1], W[2]: fp32
// (BF16 false) or bf16 (true) [C_l][C_{l-1}]
template <bool BF16, bool SEG = false>
int pointconv_level_infer(const char* fn, const float* xyz, const float* new_xyz, const float* Uf, const float* Wx, int ldw,
                          const float* density, const int32_t* idx, int B, int N, int m, int ns, int L, const int32_t* widths,
                          const void* const* W, const float* const* scale, const float* const* shift, float slope, const float* nets,
                          int M, float* out, int ldo, void* stream) {
    PCL_REQUIRE(widths && W && scale && shift, "%s: null host array", fn);
    PCL_REQUIRE(L >= 1 && L <= 4, "%s: L=%d", fn, L);
    int sid = -1;
    if (SEG && (L == 2 || L == 3)) sid = pointconv_seg_shape_id(ns, L, widths[0], widths[1], widths[L - 1], M);
    else if (L == 3) sid = pointconv_shape_id(ns, L, widths[0], widths[1], widths[2], M);
    PCL_REQUIRE(sid >= 0, "%s: no kernel for ns=%d L=%d widths %d/%d/%d M=%d (%s)", fn, ns, L, widths[0], L > 1 ? widths[1] : 0,
                L > 2 ? widths[2] : 0, M, SEG ? "pcl_pointconv_seg_level_infer_supported" : "pcl_pointconv_level_infer_supported");
    PointConvArgs a;
    if (int rc = pointconv_args(fn, xyz, new_xyz, Uf, Wx, ldw, density, idx, B, N, m, L, widths, W, scale, shift, slope, nets, M, out, ldo, a))
        return rc;
    hipStream_t st = as_stream(stream);
    if (sid == 0) return launch_pointconv<32, 3, 64, 64, 128, BF16>(fn, a, st);
    if (sid == 1) return launch_pointconv<64, 3, 128, 128, 256, BF16>(fn, a, st);
    if constexpr (SEG && BF16) {
        if (sid >= 2 && sid <= 6) return launch_pointconv_seg_bf16(sid, fn, a, st);
    } else if constexpr (SEG) {
        if (sid == 2) return launch_pointconv<32, 3, 32, 32, 64, false>(fn, a, st);
        if (sid == 3) return launch_pointconv<32, 3, 128, 128, 256, false>(fn, a, st);
        if (sid == 4) return launch_pointconv<16, 2, 256, 256, 256, false>(fn, a, st);
        if (sid == 5) return launch_pointconv<16, 2, 128, 128, 128, false>(fn, a, st);
        if (sid == 6) return launch_pointconv<16, 3, 128, 128, 128, false>(fn, a, st);
    }
    return ::pcl::fail(PCL_EINVAL, "%s: shape id %d has no launch", fn, sid);
}

}  // namespace
}  // namespace pcl
using namespace pcl;

extern "C" int pcl_pointconv_level_infer_supported(int ns, int L, int C1, int C2, int C3, int M) {
    return pointconv_shape_id(ns, L, C1, C2, C3, M) >= 0;
}

extern "C" int pcl_pointconv_level_infer_group_tile(int ns, int G) {
    return (ns == 32 || ns == 64) && G >= 1 ? pointconv_group_tile(ns, G) : 0;
}

extern "C" int pcl_pointconv_level_infer_f32(const float* xyz, const float* new_xyz, const float* Uf, const float* Wx, int ldw,
                                             const float* density, const int32_t* idx, int B, int N, int m, int ns, int L,
                                             const int32_t* widths, const float* const* W, const float* const* scale,
                                             const float* const* shift, float slope, const float* nets, int M, float* out, int ldo,
                                             void* stream) {
    return pointconv_level_infer<false>("pcl_pointconv_level_infer_f32", xyz, new_xyz, Uf, Wx, ldw, density, idx, B, N, m, ns, L, widths,
                                        reinterpret_cast<const void* const*>(W), scale, shift, slope, nets, M, out, ldo, stream);
}

extern "C" int pcl_pointconv_seg_level_infer_supported(int ns, int L, int C1, int C2, int C3, int M) {
    return pointconv_seg_shape_id(ns, L, C1, C2, C3, M) >= 0;
}

extern "C" int pcl_pointconv_seg_level_infer_group_tile(int ns, int G) {
    return (ns == 16 || ns == 32 || ns == 64) && G >= 1 ? pointconv_group_tile(ns, G) : 0;
}

extern "C" int pcl_pointconv_seg_level_infer_f32(const float* xyz, const float* new_xyz, const float* Uf, const float* Wx, int ldw,
                                                 const float* density, const int32_t* idx, int B, int N, int m, int ns, int L,
                                                 const int32_t* widths, const float* const* W, const float* const* scale,
                                                 const float* const* shift, float slope, const float* nets, int M, float* out, int ldo,
                                                 void* stream) {
    return pointconv_level_infer<false, true>("pcl_pointconv_seg_level_infer_f32", xyz, new_xyz, Uf, Wx, ldw, density, idx, B, N, m, ns, L,
                                              widths, reinterpret_cast<const void* const*>(W), scale, shift, slope, nets, M, out, ldo,
                                              stream);
}

extern "C" int pcl_pointconv_level_infer_bf16_f32(const float* xyz, const float* new_xyz, const float* Uf, const float* Wx, int ldw,
                                                  const float* density, const int32_t* idx, int B, int N, int m, int ns, int L,
                                                  const int32_t* widths, const void* const* W, const float* const* scale,
                                                  const float* const* shift, float slope, const float* nets, int M, float* out, int ldo,
                                                  void* stream) {
    return pointconv_level_infer<true>("pcl_pointconv_level_infer_bf16_f32", xyz, new_xyz, Uf, Wx, ldw, density, idx, B, N, m, ns, L,
                                       widths, W, scale, shift, slope, nets, M, out, ldo, stream);
}

extern "C" int pcl_pointconv_seg_level_infer_bf16_f32(const float* xyz, const float* new_xyz, const float* Uf, const float* Wx, int ldw,
                                                      const float* density, const int32_t* idx, int B, int N, int m, int ns, int L,
                                                      const int32_t* widths, const void* const* W, const float* const* scale,
                                                      const float* const* shift, float slope, const float* nets, int M, float* out,
                                                      int ldo, void* stream) {
    return pointconv_level_infer<true, true>("pcl_pointconv_seg_level_infer_bf16_f32", xyz, new_xyz, Uf, Wx, ldw, density, idx, B, N, m, ns,
                                             L, widths, W, scale, shift, slope, nets, M, out, ldo, stream);
}
