// infer_xconv_seg.hip -- the kernel of infer_xconv.h instantiated for the stages of networks/seg/pointcnn_partseg.py (part_num = 50)
// that fit its tile, as (K, C_mid, C2, dm):
//     (8, 64, 128, FX)    encoder_0: C = 192 channels, dm = 86 -- the FX form; the evaluator folds the taps into the pointwise weight
//     (12, 64, 128, 1)    encoder_1 and decoder_2
//     (8, 12, 25, 1)      decoder_3: C = 37 columns in ldo = 40; the gather of feat rows with an odd stride is scalar
// In a translation unit of their own so that the four instantiations of infer_xconv.hip keep their code.  The four K = 16 stages
// (C_mid = 128 and 256) have no kernel: H alone would need 135 KB and 266 KB of LDS.
#include "infer_xconv.h"

namespace pcl {
namespace xinfer {

int seg_shape_id(int K, int CM, int C2, int DM) {
    if (K == 8 && CM == 64 && C2 == 128 && DM == 0) return 0;
    if (K == 12 && CM == 64 && C2 == 128 && DM == 1) return 1;
    if (K == 8 && CM == 12 && C2 == 25 && DM == 1) return 2;
    return -1;
}

int seg_launch(int sid, const char* fn, const XArgs& a, hipStream_t st) {
    if (sid == 0) return launch<8, 64, 128, 0>(fn, a, st);
    if (sid == 1) return launch<12, 64, 128, 1>(fn, a, st);
    return launch<8, 12, 25, 1>(fn, a, st);
}

}  // namespace xinfer
}  // namespace pcl
