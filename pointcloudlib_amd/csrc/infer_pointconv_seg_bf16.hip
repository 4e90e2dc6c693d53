// infer_pointconv_seg_bf16.hip -- the bf16 instantiations of the fused PointConv level kernel (infer_pointconv.h) for the five
// part-seg shapes of pcl_pointconv_seg_level_infer_bf16_f32; the entry point, its shape table and its host checks are in
// infer_pointconv.hip.
//
// They are a file of their own because of what instantiating them beside the others does: with these five in infer_pointconv.hip the
// compiler emits other code for the existing <64, 3, 128/128/256, bf16> kernel (171 VGPRs for 169, 1955 instructions for 1951; the
// bodies share tile_layer / mfma_layer_bf16 instantiations with <32, 3, 128/128/256, bf16>, and an inlined body with several
// callers is cloned where one with a single caller is moved).  That kernel is the one in which layer 1's packed chain lost steps
// (lone()), its ISA is what was measured and tested on the GPU, and the fp32 kernels' and the two cls bf16
// kernels' ISA is to stay what it was.  Here nothing else is in the module.
#include "infer_pointconv.h"

namespace pcl {
namespace pointconv {

int launch_pointconv_seg_bf16(int sid, const char* fn, const PointConvArgs& a, hipStream_t st) {
    if (sid == 2) return launch_pointconv<32, 3, 32, 32, 64, true>(fn, a, st);
    if (sid == 3) return launch_pointconv<32, 3, 128, 128, 256, true>(fn, a, st);
    if (sid == 4) return launch_pointconv<16, 2, 256, 256, 256, true>(fn, a, st);
    if (sid == 5) return launch_pointconv<16, 2, 128, 128, 128, true>(fn, a, st);
    if (sid == 6) return launch_pointconv<16, 3, 128, 128, 128, true>(fn, a, st);
    return ::pcl::fail(PCL_EINVAL, "%s: shape id %d has no bf16 launch", fn, sid);
}

}  // namespace pointconv
}  // namespace pcl
