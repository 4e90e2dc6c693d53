// capi.hip -- library-level entry points of libpcl_hip.so (version, error string, launch helper, lab switches).
#include "common.h"
#include <math.h>
#include <string.h>
#include <atomic>

namespace pcl {
static thread_local char g_err[512] = "";
void set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
}
TimeHook& time_hook() {
    static thread_local TimeHook h = {nullptr, nullptr, "", "", ""};
    return h;
}
void set_launch_tag(const char* tag) {
    TimeHook& h = time_hook();
    strncpy(h.cur, tag ? tag : "", sizeof h.cur - 1);
    h.cur[sizeof h.cur - 1] = 0;
}
bool time_hook_matches(const TimeHook& h) { return h.want[0] == 0 || strcmp(h.want, h.cur) == 0; }
[[clang::require_constant_initialization]] LabSwitches g_lab;
int cu_count() {
    static std::atomic<int> known[16];                 // by device id, 0 = not asked yet; an id beyond the table is asked every time
    int dev = -1, cu = 0;
    const bool have = hipGetDevice(&dev) == hipSuccess;
    std::atomic<int>* slot = have && dev >= 0 && dev < 16 ? &known[dev] : nullptr;
    if (slot && (cu = slot->load(std::memory_order_relaxed)) > 0) return cu;
    if (!have || hipDeviceGetAttribute(&cu, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cu < 1) cu = 256;
    (void)hipGetLastError();
    if (slot) slot->store(cu, std::memory_order_relaxed);
    return cu;
}

}  // namespace pcl

extern "C" void pcl_time_next_launch(void* start_event, void* stop_event) {
    pcl::TimeHook& h = pcl::time_hook();
    h.start = static_cast<hipEvent_t>(start_event);
    h.stop = static_cast<hipEvent_t>(stop_event);
    h.want[0] = 0;
}

extern "C" void pcl_time_tagged_launch(void* start_event, void* stop_event, const char* tag) {
    pcl::TimeHook& h = pcl::time_hook();
    h.start = static_cast<hipEvent_t>(start_event);
    h.stop = static_cast<hipEvent_t>(stop_event);
    strncpy(h.want, tag ? tag : "", sizeof h.want - 1);
    h.want[sizeof h.want - 1] = 0;
}

// ---------------------------------------------------------------- the lab switches' setters and getters (LabSwitches, common.h)
using pcl::g_lab;
extern "C" void pcl_set_kernel_paths(int fwd_resident, int narrow_stacks, int fused_backward) {
    if (fwd_resident >= 0) g_lab.fwd_resident = fwd_resident != 0;
    if (narrow_stacks >= 0) g_lab.narrow_stacks = narrow_stacks != 0;
    if (fused_backward >= 0) g_lab.fused_backward = fused_backward != 0;
}
extern "C" void pcl_set_stack_overlap(int side_dw_on, int max_rows) {
    if (side_dw_on >= 0) g_lab.side_dw = side_dw_on != 0;
    if (max_rows > 0) g_lab.side_dw_max_rows = max_rows;
}
extern "C" int pcl_get_stack_overlap(void) { return g_lab.side_dw; }
extern "C" void pcl_set_fewrow_backward(int on) { if (on >= 0) g_lab.fewrow = on != 0; }
extern "C" int pcl_get_fewrow_backward(void) { return g_lab.fewrow; }
// 1 (opt-in; the default is 0, the fp32 MFMA): the resident-operand GEMMs take fp32 operands as three bf16 planes on the bf16 matrix pipe (nine exact partial
// products per fp32 product); 0: the fp32 MFMA form of rounds 2-3 (kept for A/B measurements and the error comparison test)
extern "C" void pcl_set_matrix_form(int split) { g_lab.split_mfma = split & 7; g_lab.split_min_k = (split >> 8) > 0 ? (split >> 8) : 128; }
extern "C" int pcl_get_matrix_form(void) { return g_lab.split_mfma; }
extern "C" void pcl_set_fb_max_blocks(int n) { g_lab.fb_cap = n; }
extern "C" void pcl_set_fb_two_images(int on) { g_lab.fb_two = on != 0; }
extern "C" int pcl_get_fb_two_images(void) { return g_lab.fb_two; }
extern "C" void pcl_set_bwd_pair(int on) { g_lab.bwd_pair = on != 0; }
extern "C" int pcl_get_bwd_pair(void) { return g_lab.bwd_pair; }
extern "C" void pcl_set_dw_tuning(int gx) { g_lab.dw_force_gx = gx > 0 ? gx : 0; }
extern "C" void pcl_set_pointconv_paths(int bwd_w_rows) { if (bwd_w_rows >= 0) g_lab.bwd_w_rows = bwd_w_rows != 0; }
extern "C" void pcl_set_scatter_form(int gather) { if (gather >= 0) g_lab.scatter_gather = gather != 0; }
extern "C" void pcl_set_fps_tuning(int threads_per_cloud, int issue_priority) {
    g_lab.fps_threads = threads_per_cloud > 0 ? threads_per_cloud : 0;
    g_lab.fps_prio = issue_priority < 0 ? 3 : issue_priority > 3 ? 3 : issue_priority;
}
extern "C" void pcl_frag_set_tuning(int max_rows, int force_tn, int force_ksw, int dw_tm, int dw_tn, int dw_ksw, int dw_ksg) {
    if (max_rows >= 0) g_lab.frag_max_rows = max_rows;
    g_lab.force_tn = force_tn; g_lab.force_ksw = force_ksw;
    g_lab.force_dw[0] = dw_tm; g_lab.force_dw[1] = dw_tn; g_lab.force_dw[2] = dw_ksw; g_lab.force_dw[3] = dw_ksg;
}
extern "C" int pcl_frag_max_rows(void) { return g_lab.frag_max_rows; }

extern "C" const char* pcl_last_launch_kernel(void) {
    const char* k = pcl::time_hook().last_kernel;
    return k ? k : "";
}

extern "C" int pcl_version(void) { return 100; }   // 0.1.0
extern "C" const char* pcl_last_error(void) { return pcl::g_err; }

// misc/ops.py:110-111: 2 ** int(math.log(batch_size)) -- natural log, as written.
extern "C" int pcl_optimal_block(int batch_size) {
    if (batch_size < 1) return 1;
    return 1 << (int)log((double)batch_size);
}
