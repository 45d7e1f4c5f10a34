// kernel_launch.hpp -- the seam between the host runtime (runtime.hip) and the kernel parts (kernel_parts.hip): the launchers the parts
// define and what a launch is described by.  No kernel lives here.  One device-side convention is here as well because both
// sides must agree on it and runtime.hip does not include the kernels: kernel_args (the runtime's self-test checks what the
// kernels assume).  (The other, the adaptive sampler's plan of a launch -- the runtime sizes the grid and the control words by the
// same ss_plan the kernel walks -- is in rt_device.hpp.)
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

#include "instances.hpp"
#include "tiles.hpp"
#include "rt_device.hpp"

using namespace glome;

// the kernel's own arguments where the dispatch put them (constant memory; the first explicit argument is at offset 0)
// (relies on the code-object ABI placing the first explicit by-value argument at offset 0 of the kernarg segment in host layout:
// checked once per process by k_kernarg_selftest, glome_ctx_create)
template <class ARGS> __device__ __forceinline__ const ARGS& kernel_args() {
  static_assert(std::is_trivially_copyable<ARGS>::value && alignof(ARGS) <= 16, "kernel_args: a by-value kernel argument in host layout");
  return *(const ARGS*)(const ARGS __attribute__((address_space(4)))*)__builtin_amdgcn_kernarg_segment_ptr();
}

// ---- a launch
// LDS carve per wave: three stack rows of cap * 64 words, or two (render_kernels.hpp lane_stack)
inline size_t flat_lds_bytes(int cap, bool two_rows = false) { return (size_t)cap * 64 * (two_rows ? 8 : 12); }
struct FlatLaunch { int grid; size_t lds; hipStream_t st; int stack_cap; uint32_t* ovf; int ovf_cap; };
struct RayStream { const float *ox, *oy, *oz, *dx, *dy, *dz, *tmax; };
struct HitStream { float* t; int32_t* prim; float *nx, *ny, *nz; int32_t* tex8; };

// ---- the adaptive sampler's plan of a launch (kSSHeads, SSPlan, ss_plan) stands beside the sampler's other item arithmetic in
// rt_device.hpp, where the CPU suite runs it too

// ---- the launchers (kernel_parts.hip; a flat launcher answers false when its part does not hold instance `key`)
bool launch_flat_p1(int key, const FlatLaunch& L, const DRenderArgs& A);
bool launch_flat_p2(int key, const FlatLaunch& L, const DRenderArgs& A);
bool launch_flat_p3(int key, const FlatLaunch& L, const DRenderArgs& A);
bool launch_flat_p4(int key, const FlatLaunch& L, const DRenderArgs& A);
bool launch_ss_flat_p5(int key, const FlatLaunch& L, const DRenderArgs& A);
bool launch_ss_flat_p9(int key, const FlatLaunch& L, const DRenderArgs& A);
void launch_render_generic(int grid, hipStream_t st, const DRenderArgs& A);        // counts bih_nodes / prim_tests (part 6)
void launch_ss_generic(int grid, hipStream_t st, const DRenderArgs& A);            // (part 7)
void launch_render_generic_lean(int grid, hipStream_t st, const DRenderArgs& A);   // does not (part 10)
void launch_ss_generic_lean(int grid, hipStream_t st, const DRenderArgs& A);       // (part 11)
void launch_rayint_batch_flat(const FlatLaunch& L, DScene S, size_t n, RayStream R, HitStream H, DCounters* c);
void launch_shadow_batch_flat(const FlatLaunch& L, DScene S, size_t n, RayStream R, uint8_t* occ, DCounters* c);
void launch_rayint_batch_generic(int grid, hipStream_t st, DScene S, size_t n, RayStream R, HitStream H, DCounters* c);
void launch_shadow_batch_generic(int grid, hipStream_t st, DScene S, size_t n, RayStream R, uint8_t* occ, DCounters* c);
void launch_inside_batch(int grid, hipStream_t st, DScene S, size_t n, const float* px, const float* py, const float* pz, uint8_t* in, DCounters* c);
// the trace seam (trace_kernels.hpp): the flat instances of parts 12-14, the generic tier's two kernels beside them
bool launch_trace_flat_p12(int key, const FlatLaunch& L, const DTraceArgs& A);
bool launch_trace_flat_p13(int key, const FlatLaunch& L, const DTraceArgs& A);
bool launch_trace_flat_p14(int key, const FlatLaunch& L, const DTraceArgs& A);
void launch_trace_generic(int grid, hipStream_t st, const DTraceArgs& A);       // counts bih_nodes / prim_tests (part 14)
void launch_trace_generic_lean(int grid, hipStream_t st, const DTraceArgs& A);  // does not (part 13)
// the lens stages of the trace seam (lens_kernels.hpp; part 15): k_camera_rays, and k_resolve staging kResolveSamplesInLds samples per pixel
// in LDS at a time -- 64 * (16 * 5 + 1) words = 20.25 KB a wave, seven waves per CU
constexpr int kResolveSamplesInLds = 16;
void launch_camera_rays(int grid, hipStream_t st, const DLensArgs& A);
void launch_resolve(int grid, hipStream_t st, const DResolveArgs& A);
// glome_render_lens_adaptive's rounds (lens_adaptive_kernels.hpp; part 15): the raygen of listed pixels, and the fold at one level -- round 0's
// (first) or a later round's -- with k_resolve's staging
void launch_camera_rays_list(int grid, hipStream_t st, const DLensListArgs& A);
void launch_adaptive_fold(int grid, hipStream_t st, bool first, const DAdaptFoldArgs& A);
