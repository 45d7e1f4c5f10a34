// mesh_update_kernels.hpp -- new vertices for a committed Mesh (glome_scene_mesh_update): what flatten.hpp's emit_mesh derives from
// the vertex arrays, made again in the scene's own pools, bit for bit what a commit of the same tree with the new arrays would upload.
// Included by runtime.hip only (light kernels of the host runtime, like bih_build_device.hpp).
//
// Everything emit_mesh derives from vertices is a (float) rounding of an fp64 expression (mtris, trinorms), a min / max of per-vertex
// values p -+ kDelta (box_of_points), or round_down / round_up of such a min / max.  x -> round_down(x - kDelta) and x ->
// round_up(x + kDelta) are monotone, so they commute with min and max: a triangle's fp32 box is folded per vertex, and every box above
// it is an fp32 min / max of boxes below.  No fp64 above the leaves, and the order of a reduction does not matter (min and max are exact;
// p -+ kDelta is never -0, so there is no tie between zeros of two signs either).
//   k_mesh_tris          one lane per mtris record: the record, its trinorms words, its fp32 box into the workspace
//   k_mesh_refit_level   one launch per tree level from the deepest up, one lane per branch node: its two boxes
//   k_mesh_bound         the box over ALL vertices (Mesh.hs:55), per block, and the check that every coordinate is finite
//   k_mesh_bound_store   folds the blocks' boxes into the mesh's header
// fp64 arithmetic is spelled with explicit round-to-nearest operations in the host's expression order (host_graph.hpp: operator-, cross,
// normalize): nothing contracts.  The library flushes fp32 subnormals, so a component whose fp32 rounding is subnormal (|x| < 2^-126)
// is stored as zero where the host stores the subnormal; every kernel reads it as zero either way.
// No kernel waits for another wave: the order between the launches is the stream's.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "flatten.hpp"

namespace glome {
namespace meshupd {

struct DTrisArgs {
  const double* verts;
  const double* norms;   // null when the mesh has none
  const int4* rows;      // two per record: (a, b, c, na) (nb, nc, trinorms base or -1, -)
  float4* mtris;         // the mesh's first record
  float4* trinorms;      // the scene's pool
  float4* ws;            // two per record: the triangle's box (lo, -) (hi, -)
  uint32_t n;            // records
};
struct DLevelArgs {
  const uint32_t* nodes; // the level's branch nodes (meshnodes indices)
  uint32_t n;
  float4* meshnodes;     // the scene's pool
  const uint4* mtrimeta; // the scene's pool
  const float4* ws;
  uint32_t first_tri;    // the record ws[0] belongs to
};
struct DBoundArgs {
  const double* verts;
  uint32_t nv;
  float4* part;          // two per block: (lo, -) (hi, -)
  unsigned int* error;   // the slot's sticky error word
};

__device__ __forceinline__ void d3_load(const double* p, int i, double v[3]) { v[0] = p[3 * (size_t)i]; v[1] = p[3 * (size_t)i + 1]; v[2] = p[3 * (size_t)i + 2]; }
// a vertex folded into an fp32 box: lo = round_down(p - kDelta), hi = round_up(p + kDelta) (box_of_points' pad, flatten.hpp's roundings)
__device__ __forceinline__ void box_add(const double p[3], float lo[3], float hi[3]) {
  for (int a = 0; a < 3; a++) { lo[a] = fminf(lo[a], round_down(__dsub_rn(p[a], kDelta))); hi[a] = fmaxf(hi[a], round_up(__dadd_rn(p[a], kDelta))); }
}

// A triangle's record (p1, n.x) (e1, n.y) (e2, n.z) from its vertices: emit_mesh's and emit_tri's expression (flatten.hpp), in the host's
// order, rounded once.  Shared with the triangle bih's update (bih_update_kernels.hpp).
__device__ __forceinline__ void tri_record(const double a[3], const double b[3], const double c[3], float4 rec[3]) {
  double e1[3], e2[3], n[3];
  for (int k = 0; k < 3; k++) { e1[k] = __dsub_rn(b[k], a[k]); e2[k] = __dsub_rn(c[k], a[k]); }
  n[0] = __dsub_rn(__dmul_rn(e1[1], e2[2]), __dmul_rn(e1[2], e2[1]));  // cross, host_graph.hpp
  n[1] = __dsub_rn(__dmul_rn(e1[2], e2[0]), __dmul_rn(e1[0], e2[2]));
  n[2] = __dsub_rn(__dmul_rn(e1[0], e2[1]), __dmul_rn(e1[1], e2[0]));
  const double inv = __ddiv_rn(1.0, __dsqrt_rn(__dadd_rn(__dadd_rn(__dmul_rn(n[0], n[0]), __dmul_rn(n[1], n[1])), __dmul_rn(n[2], n[2]))));  // normalize
  rec[0] = make_float4((float)a[0], (float)a[1], (float)a[2], (float)__dmul_rn(n[0], inv));
  rec[1] = make_float4((float)e1[0], (float)e1[1], (float)e1[2], (float)__dmul_rn(n[1], inv));
  rec[2] = make_float4((float)e2[0], (float)e2[1], (float)e2[2], (float)__dmul_rn(n[2], inv));
}

// Grid-stride over 64-record items, like k_camera_rays.
__global__ void __launch_bounds__(64) k_mesh_tris(DTrisArgs A) {
  const uint32_t items = (A.n + 63u) >> 6;
  for (uint32_t item = blockIdx.x; item < items; item += gridDim.x) {
    const uint32_t j = item * 64u + threadIdx.x;
    if (j >= A.n) continue;
    const int4 r0 = A.rows[2 * (size_t)j], r1 = A.rows[2 * (size_t)j + 1];
    if (r0.x < 0) continue;  // the placeholder of an empty leaf: no triangle, and no leaf folds its box
    double a[3], b[3], c[3];
    d3_load(A.verts, r0.x, a); d3_load(A.verts, r0.y, b); d3_load(A.verts, r0.z, c);
    float4 rec[3];
    tri_record(a, b, c, rec);
    float4* o = A.mtris + 3 * (size_t)j;
    o[0] = rec[0]; o[1] = rec[1]; o[2] = rec[2];
    if (r1.z >= 0) {
      const int ni[3] = {r0.w, r1.x, r1.y};
      for (int k = 0; k < 3; k++) { double v[3]; d3_load(A.norms, ni[k], v); A.trinorms[(size_t)r1.z + k] = make_float4((float)v[0], (float)v[1], (float)v[2], 0.0f); }
    }
    const float inf = __builtin_huge_valf();
    float lo[3] = {inf, inf, inf}, hi[3] = {-inf, -inf, -inf};
    box_add(a, lo, hi); box_add(b, lo, hi); box_add(c, lo, hi);
    A.ws[2 * (size_t)j] = make_float4(lo[0], lo[1], lo[2], 0.0f);
    A.ws[2 * (size_t)j + 1] = make_float4(hi[0], hi[1], hi[2], 0.0f);
  }
}

// A child's box.  A leaf: the fold of its triangles' boxes from the empty box -- box_empty, +-kInfinity: what MeshBuild::join starts
// from, and what an empty leaf keeps; a leaf reference's count saturates at 15, the true count is then in mtrimeta[first].z
// (rt_device.hpp mesh_closest).  A branch: the union of its node's two boxes, which the launch before this one has refitted.
__device__ __forceinline__ void child_box(const DLevelArgs& A, uint32_t ref, float lo[3], float hi[3]) {
  if (ref & 0x80000000u) {
    const uint32_t first = ref & 0x07ffffffu;
    uint32_t count = (ref >> 27) & 15u;
    if (count == 15u) count = A.mtrimeta[first].z;
    for (int a = 0; a < 3; a++) { lo[a] = (float)kInfinity; hi[a] = -(float)kInfinity; }
    const float4* w = A.ws + 2 * (size_t)(first - A.first_tri);
    for (uint32_t q = 0; q < count; q++) {
      const float4 l = w[2 * (size_t)q], h = w[2 * (size_t)q + 1];
      lo[0] = fminf(lo[0], l.x); lo[1] = fminf(lo[1], l.y); lo[2] = fminf(lo[2], l.z);
      hi[0] = fmaxf(hi[0], h.x); hi[1] = fmaxf(hi[1], h.y); hi[2] = fmaxf(hi[2], h.z);
    }
  } else {
    const float4* c = A.meshnodes + 4 * (size_t)ref;
    const float4 l0 = c[0], h0 = c[1], l1 = c[2], h1 = c[3];
    lo[0] = fminf(l0.x, l1.x); lo[1] = fminf(l0.y, l1.y); lo[2] = fminf(l0.z, l1.z);
    hi[0] = fmaxf(h0.x, h1.x); hi[1] = fmaxf(h0.y, h1.y); hi[2] = fmaxf(h0.z, h1.z);
  }
}
__global__ void __launch_bounds__(64) k_mesh_refit_level(DLevelArgs A) {
  const uint32_t items = (A.n + 63u) >> 6;
  for (uint32_t item = blockIdx.x; item < items; item += gridDim.x) {
    const uint32_t j = item * 64u + threadIdx.x;
    if (j >= A.n) continue;
    float4* o = A.meshnodes + 4 * (size_t)A.nodes[j];
    for (int side = 0; side < 2; side++) {
      const float4 w0 = o[2 * side], w1 = o[2 * side + 1];
      float lo[3], hi[3];
      child_box(A, __float_as_uint(w0.w), lo, hi);
      o[2 * side] = make_float4(lo[0], lo[1], lo[2], w0.w);  // (the child reference: the bits it had)
      o[2 * side + 1] = make_float4(hi[0], hi[1], hi[2], w1.w);
    }
  }
}

// The box over all vertices, unreferenced ones included.  A block of 256 lanes strides over the vertices, folds across each wave in
// registers and across its four waves through LDS, and stores one partial box; k_mesh_bound_store folds the partial boxes.  A lane
// that meets a coordinate that is not finite ORs kErrBadVertex into the slot's error word (glome_ctx_synchronize reports it).
constexpr int kBoundBlock = 256, kBoundMaxBlocks = 1024;
__device__ __forceinline__ void wave_fold(float lo[3], float hi[3]) {
  for (int d = 32; d >= 1; d >>= 1)
    for (int a = 0; a < 3; a++) { lo[a] = fminf(lo[a], __shfl_xor(lo[a], d, 64)); hi[a] = fmaxf(hi[a], __shfl_xor(hi[a], d, 64)); }
}
__global__ void __launch_bounds__(kBoundBlock) k_mesh_bound(DBoundArgs A) {
  __shared__ float sh[kBoundBlock / 64][6];
  const float inf = __builtin_huge_valf();
  float lo[3] = {inf, inf, inf}, hi[3] = {-inf, -inf, -inf};
  bool bad = false;
  for (uint32_t i = blockIdx.x * kBoundBlock + threadIdx.x; i < A.nv; i += gridDim.x * kBoundBlock) {
    double p[3];
    d3_load(A.verts, (int)i, p);
    bad = bad || !(isfinite(p[0]) && isfinite(p[1]) && isfinite(p[2]));
    box_add(p, lo, hi);
  }
  if (bad) atomicOr(A.error, kErrBadVertex);
  wave_fold(lo, hi);
  if ((threadIdx.x & 63) == 0) for (int a = 0; a < 3; a++) { sh[threadIdx.x >> 6][a] = lo[a]; sh[threadIdx.x >> 6][3 + a] = hi[a]; }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < kBoundBlock / 64; w++) for (int a = 0; a < 3; a++) { lo[a] = fminf(lo[a], sh[w][a]); hi[a] = fmaxf(hi[a], sh[w][3 + a]); }
    A.part[2 * (size_t)blockIdx.x] = make_float4(lo[0], lo[1], lo[2], 0.0f);
    A.part[2 * (size_t)blockIdx.x + 1] = make_float4(hi[0], hi[1], hi[2], 0.0f);
  }
}
// one wave: the partial boxes into the mesh's two header words; .w (the root reference, the unused word) keeps its bits
__global__ void __launch_bounds__(64) k_mesh_bound_store(const float4* part, uint32_t nparts, float4* hdr) {
  const float inf = __builtin_huge_valf();
  float lo[3] = {inf, inf, inf}, hi[3] = {-inf, -inf, -inf};
  for (uint32_t i = threadIdx.x; i < nparts; i += 64u) {
    const float4 l = part[2 * (size_t)i], h = part[2 * (size_t)i + 1];
    lo[0] = fminf(lo[0], l.x); lo[1] = fminf(lo[1], l.y); lo[2] = fminf(lo[2], l.z);
    hi[0] = fmaxf(hi[0], h.x); hi[1] = fmaxf(hi[1], h.y); hi[2] = fmaxf(hi[2], h.z);
  }
  wave_fold(lo, hi);
  if (threadIdx.x == 0) {
    hdr[0] = make_float4(lo[0], lo[1], lo[2], hdr[0].w);
    hdr[1] = make_float4(hi[0], hi[1], hi[2], hdr[1].w);
  }
}

}  // namespace meshupd
}  // namespace glome
