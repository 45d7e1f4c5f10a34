// kernel_parts.hip -- the kernel instances of the library, cut into parts that compile in parallel: -DGLOME_PART=k (k = 1..kParts-1,
// glome_amd/build.py) keeps the instances instances.hpp lists for part k and defines the launcher that knows them (kernel_launch.hpp).
// The device code itself is render_kernels.hpp, trace_kernels.hpp, lens_kernels.hpp and lens_adaptive_kernels.hpp; the host runtime (runtime.hip) is a unit of its own and holds none of it.
#include "render_kernels.hpp"
#include "trace_kernels.hpp"
#include "lens_kernels.hpp"
#include "lens_adaptive_kernels.hpp"

#if !defined(GLOME_PART) || GLOME_PART < 1 || GLOME_PART >= GLOME_NPARTS
#error "kernel_parts.hip is compiled once per part: -DGLOME_PART=k with k = 1..GLOME_NPARTS-1 (instances.hpp)"
#endif
#define GLOME_IN_PART(k) (GLOME_PART == (k))

// ------------------------------------------------------------------------------------------------ the generic tier's batch seams
// (not templates: defined here, in one part, and not in the header)
#if GLOME_IN_PART(8)
__global__ void __launch_bounds__(64, GLOME_GENERIC_LB) k_rayint_batch_generic(DScene, size_t n, RayStream R, HitStream H, DCounters* c) {
  const DScene& S = kernel_args<DScene>();
  Cnt cnt; unsigned int err = 0; uint32_t vm[kVmWords];
  LaneStack nopk{}; nopk.cap = 0; nopk.ovf_cap = 0;  // (the ray-batch seams walk lane by lane)
  GenericTier T{S, nullptr, 0, cnt, err, vm, nopk};
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
    store_hit(H, i, T.closest(load_ray(R, i), R.tmax[i]), (int)S.tex_bits);
  if (T.err) atomicOr(&c->error, 1u);
}
__global__ void __launch_bounds__(64, GLOME_GENERIC_LB) k_shadow_batch_generic(DScene, size_t n, RayStream R, uint8_t* occ, DCounters* c) {
  const DScene& S = kernel_args<DScene>();
  Cnt cnt; unsigned int err = 0; uint32_t vm[kVmWords];
  LaneStack nopk{}; nopk.cap = 0; nopk.ovf_cap = 0;  // (the ray-batch seams walk lane by lane)
  GenericTier T{S, nullptr, 0, cnt, err, vm, nopk};
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
    occ[i] = T.occluded(load_ray(R, i), R.tmax[i]) ? 1 : 0;
  if (T.err) atomicOr(&c->error, 1u);
}
__global__ void __launch_bounds__(64, GLOME_GENERIC_LB) k_inside_batch(DScene, size_t n, const float* px, const float* py, const float* pz, uint8_t* in, DCounters* c) {
  const DScene& S = kernel_args<DScene>();
  unsigned int err = 0;
  uint32_t vm[kVmWords];
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
    in[i] = vm_inside(S, err, vm, 0, ldu4(S.recs, S.root_rec), v3(px[i], py[i], pz[i])) ? 1 : 0;
  if (err) atomicOr(&c->error, 1u);
}
#endif

// ------------------------------------------------------------------------------------------------ launchers by part
#define GLOME_TRY_RENDER_FLAT(F, C, U, K, B, T)                                                                                                   \
  if (key == render_flat_key(F, C, U, K, B, T)) {                                                                                                 \
    hipLaunchKernelGGL((k_render_flat<F, C, U, K, B, T>), dim3(L.grid), dim3(64), L.lds, L.st, A, L.stack_cap, L.ovf, L.ovf_cap);                 \
    return true;                                                                                                                                  \
  }
#define GLOME_TRY_SS_FLAT(U, K, B, T, F)                                                                                                          \
  if (key == ss_flat_key(U, K, B, T, F)) {                                                                                                        \
    hipLaunchKernelGGL((k_ss_frame_flat<U, K, B, T, F>), dim3(L.grid), dim3(64), L.lds, L.st, A, L.stack_cap, L.ovf, L.ovf_cap);                  \
    return true;                                                                                                                                  \
  }
#if GLOME_IN_PART(1)
bool launch_flat_p1(int key, const FlatLaunch& L, const DRenderArgs& A) { GLOME_RENDER_FLAT_P1(GLOME_TRY_RENDER_FLAT) return false; }
#endif
#if GLOME_IN_PART(2)
bool launch_flat_p2(int key, const FlatLaunch& L, const DRenderArgs& A) { GLOME_RENDER_FLAT_P2(GLOME_TRY_RENDER_FLAT) return false; }
#endif
#if GLOME_IN_PART(3)
bool launch_flat_p3(int key, const FlatLaunch& L, const DRenderArgs& A) { GLOME_RENDER_FLAT_P3(GLOME_TRY_RENDER_FLAT) return false; }
#endif
#if GLOME_IN_PART(4)
bool launch_flat_p4(int key, const FlatLaunch& L, const DRenderArgs& A) { GLOME_RENDER_FLAT_P4(GLOME_TRY_RENDER_FLAT) return false; }
#endif
#if GLOME_IN_PART(5)
bool launch_ss_flat_p5(int key, const FlatLaunch& L, const DRenderArgs& A) { GLOME_SS_FLAT_P5(GLOME_TRY_SS_FLAT) return false; }
void launch_rayint_batch_flat(const FlatLaunch& L, DScene S, size_t n, RayStream R, HitStream H, DCounters* c) {
  hipLaunchKernelGGL((k_rayint_batch_flat<false>), dim3(L.grid), dim3(64), L.lds, L.st, S, n, R, H, L.stack_cap, L.ovf, L.ovf_cap, c);
}
void launch_shadow_batch_flat(const FlatLaunch& L, DScene S, size_t n, RayStream R, uint8_t* occ, DCounters* c) {
  hipLaunchKernelGGL((k_shadow_batch_flat<0>), dim3(L.grid), dim3(64), L.lds, L.st, S, n, R, occ, L.stack_cap, L.ovf, L.ovf_cap, c);
}
#endif
#if GLOME_IN_PART(9)
bool launch_ss_flat_p9(int key, const FlatLaunch& L, const DRenderArgs& A) { GLOME_SS_FLAT_P9(GLOME_TRY_SS_FLAT) return false; }
#endif
#if GLOME_IN_PART(6)
void launch_render_generic(int grid, hipStream_t st, const DRenderArgs& A) { hipLaunchKernelGGL(k_render_generic<true>, dim3(grid), dim3(64), flat_lds_bytes((int)A.S.pk_generic_cap), st, A); }
#endif
#if GLOME_IN_PART(7)
void launch_ss_generic(int grid, hipStream_t st, const DRenderArgs& A) { hipLaunchKernelGGL(k_ss_frame_generic<true>, dim3(grid), dim3(64), flat_lds_bytes((int)A.S.pk_generic_cap), st, A); }
#endif
#if GLOME_IN_PART(10)
void launch_render_generic_lean(int grid, hipStream_t st, const DRenderArgs& A) { hipLaunchKernelGGL(k_render_generic<false>, dim3(grid), dim3(64), flat_lds_bytes((int)A.S.pk_generic_cap), st, A); }
#endif
#if GLOME_IN_PART(11)
void launch_ss_generic_lean(int grid, hipStream_t st, const DRenderArgs& A) { hipLaunchKernelGGL(k_ss_frame_generic<false>, dim3(grid), dim3(64), flat_lds_bytes((int)A.S.pk_generic_cap), st, A); }
#endif
#if GLOME_IN_PART(8)
void launch_rayint_batch_generic(int grid, hipStream_t st, DScene S, size_t n, RayStream R, HitStream H, DCounters* c) { hipLaunchKernelGGL(k_rayint_batch_generic, dim3(grid), dim3(64), 0, st, S, n, R, H, c); }
void launch_shadow_batch_generic(int grid, hipStream_t st, DScene S, size_t n, RayStream R, uint8_t* occ, DCounters* c) { hipLaunchKernelGGL(k_shadow_batch_generic, dim3(grid), dim3(64), 0, st, S, n, R, occ, c); }
void launch_inside_batch(int grid, hipStream_t st, DScene S, size_t n, const float* px, const float* py, const float* pz, uint8_t* in, DCounters* c) {
  hipLaunchKernelGGL(k_inside_batch, dim3(grid), dim3(64), 0, st, S, n, px, py, pz, in, c);
}
#endif
// the trace seam
#define GLOME_TRY_TRACE_FLAT(F, C, U, K, B)                                                                                                       \
  if (key == render_flat_key(F, C, U, K, B, false)) {                                                                                             \
    hipLaunchKernelGGL((k_trace_batch_flat<F, C, U, K, B>), dim3(L.grid), dim3(64), L.lds, L.st, A, L.stack_cap, L.ovf, L.ovf_cap);               \
    return true;                                                                                                                                  \
  }
#if GLOME_IN_PART(12)
bool launch_trace_flat_p12(int key, const FlatLaunch& L, const DTraceArgs& A) { GLOME_TRACE_FLAT_P12(GLOME_TRY_TRACE_FLAT) return false; }
#endif
#if GLOME_IN_PART(13)
bool launch_trace_flat_p13(int key, const FlatLaunch& L, const DTraceArgs& A) { GLOME_TRACE_FLAT_P13(GLOME_TRY_TRACE_FLAT) return false; }
void launch_trace_generic_lean(int grid, hipStream_t st, const DTraceArgs& A) { hipLaunchKernelGGL(k_trace_batch_generic<false>, dim3(grid), dim3(64), flat_lds_bytes((int)A.S.pk_generic_cap), st, A); }
#endif
#if GLOME_IN_PART(14)
bool launch_trace_flat_p14(int key, const FlatLaunch& L, const DTraceArgs& A) { GLOME_TRACE_FLAT_P14(GLOME_TRY_TRACE_FLAT) return false; }
void launch_trace_generic(int grid, hipStream_t st, const DTraceArgs& A) { hipLaunchKernelGGL(k_trace_batch_generic<true>, dim3(grid), dim3(64), flat_lds_bytes((int)A.S.pk_generic_cap), st, A); }
#endif
// the lens stages of the trace seam (lens_kernels.hpp): plain grids, the arguments by value
#if GLOME_IN_PART(15)
void launch_camera_rays(int grid, hipStream_t st, const DLensArgs& A) { hipLaunchKernelGGL(k_camera_rays<>, dim3(grid), dim3(64), 0, st, A); }
void launch_resolve(int grid, hipStream_t st, const DResolveArgs& A) { hipLaunchKernelGGL(k_resolve<kResolveSamplesInLds>, dim3(grid), dim3(64), 0, st, A); }
// glome_render_lens_adaptive's rounds (lens_adaptive_kernels.hpp)
void launch_camera_rays_list(int grid, hipStream_t st, const DLensListArgs& A) { hipLaunchKernelGGL(k_camera_rays_list<>, dim3(grid), dim3(64), 0, st, A); }
void launch_adaptive_fold(int grid, hipStream_t st, bool first, const DAdaptFoldArgs& A) {
  if (first) hipLaunchKernelGGL((k_adaptive_fold<kResolveSamplesInLds, true>), dim3(grid), dim3(64), 0, st, A);
  else hipLaunchKernelGGL((k_adaptive_fold<kResolveSamplesInLds, false>), dim3(grid), dim3(64), 0, st, A);
}
#endif
