// common.h -- shared helpers for the gfx950 kernels of libpcl_hip.so.
// Wave = 64 lanes everywhere (CDNA4); no other target is supported.
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <stdint.h>
#include <stdio.h>
#include <stdarg.h>
#include <stdlib.h>
#include "../../include/pcl_hip.h"

namespace pcl {

void set_error(const char* fmt, ...);

inline int fail(int code, const char* fmt, ...) {
    char buf[256];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    set_error("%s", buf);
    return code;
}

inline int check_launch(const char* what) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(PCL_EHIP, "%s: %s", what, hipGetErrorString(e));
    return PCL_OK;
}

#define PCL_REQUIRE(cond, ...) \
    do { if (!(cond)) return ::pcl::fail(PCL_EINVAL, __VA_ARGS__); } while (0)

// Every entry point converts its `void* stream` exactly once, before launching: we use that moment to drop a
// stale sticky error left by somebody else's HIP call in this thread, so check_launch() reports only ours.
static inline hipStream_t as_stream(void* s) {
    (void)hipGetLastError();
    return reinterpret_cast<hipStream_t>(s);
}

// Measurement hook (bench.py): pcl_time_next_launch(start, stop) arms two HIP events for the next GEMM-family kernel this
// thread launches; they receive the kernel's own begin / end timestamps (the dispatch packet's, what rocprofv3 reports)
// instead of the times two marker packets around the call would see.  Unarmed (normal operation) it is a plain launch.
// Inside a per-stack entry point (stack.hip) many such kernels are launched by ONE call: each carries a launch tag
// ("fb256x128", "fwd128x256", ...; set_launch_tag) and pcl_time_tagged_launch arms the events for the next launch whose tag
// matches (an empty wanted tag matches anything).
struct TimeHook { hipEvent_t start, stop; char want[32]; char cur[32]; const char* last_kernel; };
TimeHook& time_hook();
// Lab switches: every process-wide value that selects a kernel path or tunes a launch shape (DESIGN.md section 1 has the table).
// The contract, once: the values are process-wide, changed only through the setters in capi.hip (C calls -- the library reads no
// environment variables) BETWEEN calls of the library, and read unsynchronised by every call; several size queries answer by
// them, so a host-side cache of such an answer is dropped whenever a setter runs (pointcloudlib_amd/_lib.py).
struct LabSwitches {
    int fwd_resident = 1, narrow_stacks = 1, fused_backward = 1;   // pcl_set_kernel_paths: resident-weight forward, recompute-per-pass narrow stacks, fused dX + dW backward
    int side_dw = 0, side_dw_max_rows = 8192;                      // pcl_set_stack_overlap: few-row stacks' dW launches on the library's second stream
    int fewrow = 0;                                                // pcl_set_fewrow_backward: constants + dy in one launch, dX and dW on the formed dy
    int split_mfma = 0, split_min_k = 128;                         // pcl_set_matrix_form: 0 = fp32 MFMA; bit 0 the resident-operand forward, bit 1 the staged GEMMs with K >= split_min_k as three bf16 planes
    int fb_cap = 0;                                                // pcl_set_fb_max_blocks: cap on the fused backward's persistent grid (0 = one workgroup per CU)
    int fb_two = 1;                                                // pcl_set_fb_two_images: the fused backward's 128 x 64 shape on two tile images
    int bwd_pair = 1;                                              // pcl_set_bwd_pair: 0 = the two launches + reduce of rounds 1-5
    int dw_force_gx = 0;                                           // pcl_set_dw_tuning: row-chunk workgroups per output tile of the plain-dy dW (0 = the library's choice)
    int bwd_w_rows = 1;                                            // pcl_set_pointconv_paths: PointConv weight gradient with the row-major LDS image
    int scatter_gather = 1;                                        // pcl_set_scatter_form: 0 = the fp32-atomic scatter everywhere
    int fps_threads = 0, fps_prio = 3;                             // pcl_set_fps_tuning: threads per cloud (0 = by N), issue priority
    int frag_max_rows = 8192;                                      // pcl_frag_set_tuning: largest P for which a plain stack takes the fragment kernels ...
    int force_tn = 0, force_ksw = 0, force_dw[4] = {0, 0, 0, 0};   // ... and its lab / test knobs (0 = the library's choice): column tiles, row groups, dW tm / tn / ksw / ksg
};
extern LabSwitches g_lab;
void set_launch_tag(const char* tag);
bool time_hook_matches(const TimeHook& h);
#define PCL_LAUNCH_TIMED_LDS(kernel, grid, blk, lds, st, ...)                                                          \
    do {                                                                                                                \
        ::pcl::TimeHook& h_ = ::pcl::time_hook();                                                                       \
        h_.last_kernel = #kernel;    /* pcl_last_launch_kernel(): which kernel an entry point chose (profiling tools) */ \
        if (h_.start && ::pcl::time_hook_matches(h_)) {                                                                 \
            hipExtLaunchKernelGGL(kernel, grid, blk, lds, st, h_.start, h_.stop, 0, __VA_ARGS__);                       \
            h_.start = h_.stop = nullptr;                                                                               \
        } else hipLaunchKernelGGL(kernel, grid, blk, lds, st, __VA_ARGS__);                                             \
    } while (0)
#define PCL_LAUNCH_TIMED(kernel, grid, blk, st, ...) PCL_LAUNCH_TIMED_LDS(kernel, grid, blk, 0, st, __VA_ARGS__)

// ---------------------------------------------------------------- host launch helpers
// CU count of the CURRENT device, asked once per device id (capi.hip).  256 -- the MI355X's own count -- when there is no device or
// the query fails; the sticky HIP error of the failed query is cleared (the size queries answer without a GPU).
int cu_count();

// Dynamic LDS beyond the 64 KB a kernel may use by default needs the kernel's limit raised first: call this before every such
// launch (a no-op up to 64 KB; the attribute belongs to the current device, so nothing is remembered here).
template <class K>
inline int lds_opt_in(K* kernel, size_t bytes, const char* who) {
    if (bytes <= 64 * 1024) return PCL_OK;
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    if (e != hipSuccess) return fail(PCL_EHIP, "%s: hipFuncSetAttribute(%zu): %s", who, bytes, hipGetErrorString(e));
    return PCL_OK;
}

// May a kernel move 16-byte pieces of these operands?  True when every pointer given is 16-byte aligned; null counts as aligned.
template <class... T>
inline bool al16(const T*... p) { return ((uintptr_t(0) | ... | reinterpret_cast<uintptr_t>(p)) & 15) == 0; }

// XCD-aware logical block id for a 1-D grid whose consecutive blocks walk the clouds one after another (`bpc` blocks per
// cloud, nblk = clouds * bpc).  The hardware deals consecutive workgroup ids to the 8 XCDs round-robin, each with its own
// 4 MB L2: with the plain id every XCD touches every cloud's table.  Here XCD j takes the clouds j, j+8, ... whole, one
// after the other, so a cloud's table is gathered by workgroups that share an L2.  Identity when the shape does not divide.
__device__ __forceinline__ unsigned xcd_cloud_block(unsigned lin, unsigned nblk, unsigned bpc) {
    if (bpc == 0 || nblk % (8u * bpc) != 0) return lin;
    const unsigned slot = lin >> 3;
    return ((lin & 7u) + 8u * (slot / bpc)) * bpc + slot % bpc;
}

// ---------------------------------------------------------------- device helpers
#define PCL_WAVE 64

// Single-rounded fp32 ops: index-producing kernels must evaluate distances exactly as the source
// text of the reference writes them (no FMA contraction), whatever the compiler flags.
__device__ __forceinline__ float sq_dist3(float ax, float ay, float az, float bx, float by, float bz) {
    // (ax-bx)*(ax-bx) + (ay-by)*(ay-by) + (az-bz)*(az-bz), left to right
    const float dx = __fsub_rn(ax, bx), dy = __fsub_rn(ay, by), dz = __fsub_rn(az, bz);
    return __fadd_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)), __fmul_rn(dz, dz));
}

template <int CTRL>
__device__ __forceinline__ unsigned dpp_u32(unsigned v, unsigned old) {
    return (unsigned)__builtin_amdgcn_update_dpp((int)old, (int)v, CTRL, 0xf, 0xf, false);
}

// Wave-wide max / min of a 32-bit unsigned value; result is wave-uniform (SGPR).
// 4 DPP steps reduce each row of 16 lanes, 4 readlanes + scalar ops combine the rows.
__device__ __forceinline__ unsigned wave_max_u32(unsigned v) {
    v = max(v, dpp_u32<0xB1>(v, v));    // quad_perm [1,0,3,2]
    v = max(v, dpp_u32<0x4E>(v, v));    // quad_perm [2,3,0,1]
    v = max(v, dpp_u32<0x141>(v, v));   // row_half_mirror
    v = max(v, dpp_u32<0x140>(v, v));   // row_mirror
    const unsigned a = __builtin_amdgcn_readlane(v, 0), b = __builtin_amdgcn_readlane(v, 16);
    const unsigned c = __builtin_amdgcn_readlane(v, 32), d = __builtin_amdgcn_readlane(v, 48);
    return max(max(a, b), max(c, d));
}
__device__ __forceinline__ unsigned wave_min_u32(unsigned v) {
    v = min(v, dpp_u32<0xB1>(v, v));
    v = min(v, dpp_u32<0x4E>(v, v));
    v = min(v, dpp_u32<0x141>(v, v));
    v = min(v, dpp_u32<0x140>(v, v));
    const unsigned a = __builtin_amdgcn_readlane(v, 0), b = __builtin_amdgcn_readlane(v, 16);
    const unsigned c = __builtin_amdgcn_readlane(v, 32), d = __builtin_amdgcn_readlane(v, 48);
    return min(min(a, b), min(c, d));
}

// A thread's walk over the rows r, r + step, ... < n with U rows requested before the first is used: use(q, load(q)) runs in ascending
// q exactly as the one-load-per-trip loop would, so whatever it accumulates or compares comes out the same bits -- but a trip costs
// one memory round trip per U rows instead of one per row.  (The plain loop compiles to load, wait for it, use, branch: the compiler
// does not hoist the next trip's load across the loop-carried compare or add.)  Fewer than U rows left: batches of U/2, U/4, .. 1,
// each at most once -- no padding, no row touched that the plain loop would not touch.
template <int U, class L, class F>
__device__ __forceinline__ void rows_in_flight(int r, int step, int n, L&& load, F&& use) {
    for (; r + (U - 1) * step < n; r += U * step) {
        decltype(load(r)) v[U];
#pragma unroll
        for (int u = 0; u < U; ++u) v[u] = load(r + u * step);
#pragma unroll
        for (int u = 0; u < U; ++u) use(r + u * step, v[u]);
    }
    if constexpr (U > 1) rows_in_flight<U / 2>(r, step, n, load, use);
}
// the same over one column x[q * ld]
template <int U, class T, class F>
__device__ __forceinline__ void rows_in_flight(const T* __restrict__ x, size_t ld, int r, int step, int n, F&& use) {
    rows_in_flight<U>(r, step, n, [&](int q) { return x[(size_t)q * ld]; }, use);
}
__device__ __forceinline__ int lane_id() { return (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u)); }

// number of set bits of `mask` strictly below this lane
__device__ __forceinline__ int mbcnt(unsigned long long mask) {
    return (int)__builtin_amdgcn_mbcnt_hi((unsigned)(mask >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mask, 0u));
}

}  // namespace pcl
