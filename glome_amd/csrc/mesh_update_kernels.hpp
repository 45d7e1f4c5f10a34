// mesh_update_kernels.hpp -- new vertices for a committed Mesh (glome_scene_mesh_update): what flatten.hpp's emit_mesh derives from
// the vertex arrays, made again in the scene's own pools, bit for bit what a commit of the same tree with the new arrays would upload.
// Included by runtime.hip only (light kernels of the host runtime, like bih_build_device.hpp).
//
// Everything emit_mesh derives from vertices is a (float) rounding of an fp64 expression (mtris, trinorms), a min / max of per-vertex
// values p -+ kDelta (box_of_points), or round_down / round_up of such a min / max.  x -> round_down(x - kDelta) and x ->
// round_up(x + kDelta) are monotone, so they commute with min and max: a triangle's fp32 box is folded per vertex, and every box above
// it is an fp32 min / max of boxes below.  No fp64 above the leaves, and the order of a reduction does not matter (min and max are exact;
// p -+ kDelta is never -0, so there is no tie between zeros of two signs either).
//   k_mesh_tris          one lane per mtris record: the record, its trinorms words, its fp32 box into the workspace; an instance per
//                        point source (fp64 or fp32 arrays), one body after the load
//   k_mesh_refit_level   one launch per tree level from the deepest up, one lane per branch node: its two boxes
// and, of update_common.hpp, with real infinity as the start:
//   k_points_bound       the box over ALL vertices (Mesh.hs:55), per block, and the check that every coordinate is finite
//   k_bound_store        folds the blocks' boxes into the mesh's header
// fp64 arithmetic is spelled with explicit round-to-nearest operations in the host's expression order (host_graph.hpp: operator-, cross,
// normalize): nothing contracts.  The library flushes fp32 subnormals, so a component whose fp32 rounding is subnormal (|x| < 2^-126)
// is stored as zero where the host stores the subnormal; every kernel reads it as zero either way.
// No kernel waits for another wave: the order between the launches is the stream's.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "flatten.hpp"
#include "update_common.hpp"

namespace glome {
namespace meshupd {

template <class Src> struct DTrisArgs {
  Src verts;             // a dense point source (update_common.hpp), fp64 or fp32: the rows below are the mesh's own index table
  Src norms;             // null when the mesh has none
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

template <class Src> __global__ void __launch_bounds__(64) k_mesh_tris(DTrisArgs<Src> A) {
  upd::for_lanes(A.n, [&](uint32_t j) {
    const int4 r0 = A.rows[2 * (size_t)j], r1 = A.rows[2 * (size_t)j + 1];
    if (r0.x < 0) return;  // the placeholder of an empty leaf: no triangle, and no leaf folds its box
    double a[3], b[3], c[3];
    A.verts.load(r0.x, a); A.verts.load(r0.y, b); A.verts.load(r0.z, c);
    float4 rec[3];
    upd::tri_record(a, b, c, rec);
    float4* o = A.mtris + 3 * (size_t)j;
    o[0] = rec[0]; o[1] = rec[1]; o[2] = rec[2];
    if (r1.z >= 0) {
      const int ni[3] = {r0.w, r1.x, r1.y};
      for (int k = 0; k < 3; k++) { double v[3]; A.norms.load(ni[k], v); A.trinorms[(size_t)r1.z + k] = make_float4((float)v[0], (float)v[1], (float)v[2], 0.0f); }
    }
    const float inf = __builtin_huge_valf();
    float lo[3] = {inf, inf, inf}, hi[3] = {-inf, -inf, -inf};
    upd::box_add(a, lo, hi); upd::box_add(b, lo, hi); upd::box_add(c, lo, hi);
    upd::store_rows(A.ws + 2 * (size_t)j, lo, hi);
  });
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
    upd::fold_rows(A.ws + 2 * (size_t)(first - A.first_tri), 0u, count, 1u, lo, hi);
  } else {
    const float4* c = A.meshnodes + 4 * (size_t)ref;
    const float4 l0 = c[0], h0 = c[1], l1 = c[2], h1 = c[3];
    lo[0] = fminf(l0.x, l1.x); lo[1] = fminf(l0.y, l1.y); lo[2] = fminf(l0.z, l1.z);
    hi[0] = fmaxf(h0.x, h1.x); hi[1] = fmaxf(h0.y, h1.y); hi[2] = fmaxf(h0.z, h1.z);
  }
}
__global__ void __launch_bounds__(64) k_mesh_refit_level(DLevelArgs A) {
  upd::for_lanes(A.n, [&](uint32_t j) {
    float4* o = A.meshnodes + 4 * (size_t)A.nodes[j];
    for (int side = 0; side < 2; side++) {
      const float4 w0 = o[2 * side], w1 = o[2 * side + 1];
      float lo[3], hi[3];
      child_box(A, __float_as_uint(w0.w), lo, hi);
      upd::store_rows(o + 2 * side, lo, hi, w0.w, w1.w);  // (.w: the child reference and the unused word, the bits they had)
    }
  });
}

}  // namespace meshupd
}  // namespace glome
