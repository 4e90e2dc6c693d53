// infer_xconv.hip -- one X-conv stage of PointCNN in evaluation mode as ONE launch: the C entry points, and the instantiations of
// the kernel of infer_xconv.h (its text, thread map and numeric contract are described there) for the four stages of
// networks/cls/pointcnn.py.  The stages of networks/seg/pointcnn_partseg.py are instantiated in infer_xconv_seg.hip.
#include "infer_xconv.h"

namespace pcl {
namespace xinfer {

// regions per workgroup: whole tiles, XI_MAXTILES of them, halved while the launch would leave compute units without a workgroup
// (K = 16: the tile's LDS admits one workgroup per compute unit) or with fewer than two (K = 8, 12)
int region_tile(int K, int R) {
    int tiles = XI_MAXTILES;
    const int want = (K == 16 ? 1 : 2) * cu_count();
    while (tiles > 1 && (R + tiles * XI_R - 1) / (tiles * XI_R) < want) tiles /= 2;
    return tiles * XI_R;
}

// the four stages of networks/cls/pointcnn.py
int shape_id(int K, int CM, int C2, int DM) {
    if (K == 8 && CM == 12 && C2 == 24 && DM == 16) return 0;
    if (K == 12 && CM == 24 && C2 == 48 && DM == 2) return 1;
    if (K == 16 && CM == 48 && C2 == 96 && DM == 2) return 2;
    if (K == 16 && CM == 96 && C2 == 192 && DM == 2) return 3;
    return -1;
}

// what the tap form and the FX form (wd = bias = nullptr, dm = 0) share: the checks and the argument block
int run(const char* fn, const char* query, const float* pts, const float* rep, const float* feat, const float* fs, const float* ft, const int32_t* knn,
        int B, int N, int P, int K, int D, int C_mid, int C2, int dm, const float* Wa, const float* sa, const float* ta, const float* Wb,
        const float* sb, const float* tb, const float* W0, const float* W1, const float* sc1, const float* sh1, const float* W2,
        const float* b2, const float* wd, const float* bias, float* out, int ldo, void* stream) {
    const int sid = dm ? shape_id(K, C_mid, C2, dm) : -1;
    const int seg = sid < 0 ? seg_shape_id(K, C_mid, C2, dm) : -1;
    PCL_REQUIRE(sid >= 0 || seg >= 0, "%s: no kernel for K=%d C_mid=%d C2=%d dm=%d (%s)", fn, K, C_mid, C2, dm, query);
    PCL_REQUIRE(pts && rep && feat && fs && ft && knn && Wa && sa && ta && Wb && sb && tb && W0 && W1 && sc1 && sh1 && W2 && b2 && out &&
                (dm == 0 || (wd && bias)), "%s: null pointer", fn);
    PCL_REQUIRE(B >= 1 && N >= 1 && P >= 1 && D >= 1, "%s: bad sizes B=%d N=%d P=%d D=%d", fn, B, N, P, D);
    PCL_REQUIRE((size_t)B * P < (1u << 31) && (size_t)B * N < (1u << 31), "%s: too many regions / points", fn);
    const int cols = (C_mid + C2) * (dm ? dm : K);
    PCL_REQUIRE(ldo >= cols && ldo % 4 == 0, "%s: ldo=%d for %d columns (a multiple of 4)", fn, ldo, cols);
    // (Wb, W0, W1, W2 and -- where dm > 1 -- out are moved in 16-byte pieces: their alignment is the caller's precondition
    // (include/pcl_hip.h), held by pointcloudlib_amd/inference.py before the call; there is no other path to choose here)
    XArgs a = {};
    a.pts = pts; a.rep = rep; a.feat = feat; a.fs = fs; a.ft = ft; a.knn = knn; a.R = B * P; a.N = N; a.P = P; a.KD = K * D; a.D = D;
    a.Wa = Wa; a.sa = sa; a.ta = ta; a.Wb = Wb; a.sb = sb; a.tb = tb;
    a.W0 = W0; a.W1 = W1; a.sc1 = sc1; a.sh1 = sh1; a.W2 = W2; a.b2 = b2; a.wd = wd; a.bias = bias; a.out = out; a.ldo = ldo;
    hipStream_t st = as_stream(stream);
    if (seg >= 0) return seg_launch(seg, fn, a, st);
    if (sid == 0) return launch<8, 12, 24, 16>(fn, a, st);
    if (sid == 1) return launch<12, 24, 48, 2>(fn, a, st);
    if (sid == 2) return launch<16, 48, 96, 2>(fn, a, st);
    return launch<16, 96, 192, 2>(fn, a, st);
}

}  // namespace xinfer
}  // namespace pcl
using namespace pcl;

extern "C" int pcl_xconv_level_infer_supported(int K, int C_mid, int C2, int dm) {
    return dm >= 1 && (xinfer::shape_id(K, C_mid, C2, dm) >= 0 || xinfer::seg_shape_id(K, C_mid, C2, dm) >= 0);
}

extern "C" int pcl_xconv_level_infer_fx_supported(int K, int C_mid, int C2) { return xinfer::seg_shape_id(K, C_mid, C2, 0) >= 0; }

extern "C" int pcl_xconv_level_infer_region_tile(int K, int R) {
    return (K == 8 || K == 12 || K == 16) && R >= 1 ? xinfer::region_tile(K, R) : 0;
}

extern "C" int pcl_xconv_level_infer_f32(const float* pts, const float* rep, const float* feat, const float* fs, const float* ft, const int32_t* knn, int B, int N, int P,
                                         int K, int D, int C_mid, int C2, int dm, const float* Wa, const float* sa, const float* ta,
                                         const float* Wb, const float* sb, const float* tb, const float* W0, const float* W1,
                                         const float* sc1, const float* sh1, const float* W2, const float* b2, const float* wd,
                                         const float* bias, float* out, int ldo, void* stream) {
    const char* fn = "pcl_xconv_level_infer_f32";
    PCL_REQUIRE(dm >= 1, "%s: no kernel for K=%d C_mid=%d C2=%d dm=%d (pcl_xconv_level_infer_supported)", fn, K, C_mid, C2, dm);
    return xinfer::run(fn, "pcl_xconv_level_infer_supported", pts, rep, feat, fs, ft, knn, B, N, P, K, D, C_mid, C2, dm, Wa, sa, ta, Wb, sb, tb,
                       W0, W1, sc1, sh1, W2, b2, wd, bias, out, ldo, stream);
}

extern "C" int pcl_xconv_level_infer_fx_f32(const float* pts, const float* rep, const float* feat, const float* fs, const float* ft, const int32_t* knn, int B, int N,
                                            int P, int K, int D, int C_mid, int C2, const float* Wa, const float* sa, const float* ta,
                                            const float* Wb, const float* sb, const float* tb, const float* W0, const float* W1,
                                            const float* sc1, const float* sh1, const float* W2, const float* b2, float* out, int ldo,
                                            void* stream) {
    return xinfer::run("pcl_xconv_level_infer_fx_f32", "pcl_xconv_level_infer_fx_supported", pts, rep, feat, fs, ft, knn, B, N, P, K, D, C_mid, C2,
                       0, Wa, sa, ta, Wb, sb, tb, W0, W1, sc1, sh1, W2, b2, nullptr, nullptr, out, ldo, stream);
}
