// bih_update_kernels.hpp -- new triangles for a committed triangle bih (glome_scene_bih_update): what flatten.hpp's emit_bih / emit_tri /
// emit_pairs derive from the items' vertices, made again in the scene's own pools, bit for bit what a commit of the same tree with the
// new triangles (glome_sb_bih_set_triangles) would upload.  Included by runtime.hip only, like mesh_update_kernels.hpp, with which it
// shares the record arithmetic (tri_record) and the bound reduction (k_points_bound) of update_common.hpp.
//
// A branch's planes are round_up(lmax + kDelta) and round_down(rmin - kDelta), lmax / rmin the max / min over a subtree of the items'
// box hi[axis] / lo[axis] from -+kInfinity, and an item's box is max(p) + kDelta / min(p) - kDelta (host_graph.hpp: bound, BihBuild::rec).
// x -> round_up((x + kDelta) + kDelta) and x -> round_down((x - kDelta) - kDelta) are monotone, so they commute with max and min: the
// value is rounded to fp32 per vertex and folded in fp32 above it, in any order, from round_up(-kInfinity + kDelta) and
// round_down(kInfinity - kDelta) -- what an empty subtree gives on the host.  A node holds two planes, not two boxes, so the pass keeps a
// box per record and per branch slot in a workspace: an ancestor may split on any axis.  The tree's own box is ONE pad deep, a different
// fp32 value: it is reduced on its own over all vertices (k_points_bound), from the host's box_empty.
//   k_bih_tris           one lane per record: the tris record, its words of its pair record, its plane-form box into the workspace; an
//                        instance per point source (update_common.hpp: dense or indexed, fp64 or fp32), one body after the load
//   k_bih_level          one launch per tree level from the deepest up, one lane per branch node: its planes, its box
//   k_bih_levels_merged  a run of narrow levels (each at most kMergeBlock nodes) in ONE block, a block barrier between levels: off by
//                        default (GLOME_DEBUG_BIH_UPDATE_MERGED) until measured to win; wide levels then keep k_bih_level
// and, of update_common.hpp, k_bound_store with (float)kInfinity as the start: k_points_bound's partial boxes into the tree's header.
// The levels and the header's store are also what an item bih's refit launches (item_bih_update_kernels.hpp).
// The library flushes fp32 subnormals: as in the mesh update, a component whose fp32 rounding is subnormal is stored as zero.
// No wave waits for a wave of another block: the order between the launches is the stream's, inside the merged launch the barrier's.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "flatten.hpp"
#include "update_common.hpp"

namespace glome {
namespace bihupd {

// The widest level the merged launch takes, and its block: the most lanes one block has (16 waves on one CU).  A level costs the merged
// launch one barrier where it costs the per-level form a launch, so the more levels fit, the better; the levels above it run as
// grid-stride launches of 64-lane blocks like the mesh update's.
constexpr int kMergeBlock = 1024;

template <class Src> struct DTrisArgs {
  Src src;               // the items' vertices, three points per item: p1 p2 p3 (update_common.hpp: a point source)
  const uint2* rows;     // per record: (item, pair words -- LeafBihUpdateInfo)
  float4* tris;          // the tree's first record
  float* tripairs;       // the scene's pool
  float4* ws;            // two per record: the triangle's plane-form box (lo, -) (hi, -)
  uint32_t n;            // records
};
struct DLevelArgs {
  const uint32_t* nodes; // branch slots (bihnodes indices), level after level, deepest first
  float4* bihnodes;      // the scene's pools
  float4* pknodes;       // null when the tree has no packet form
  const float4* ws_tri;  // two per record
  float4* ws_node;       // two per slot of the tree
  uint32_t first_rec, first_slot;
};

template <class Src> __global__ void __launch_bounds__(64) k_bih_tris(DTrisArgs<Src> A) {
  upd::for_lanes(A.n, [&](uint32_t j) {
    const uint2 row = A.rows[j];
    double a[3], b[3], c[3];
    A.src.load(3 * (int)row.x, a); A.src.load(3 * (int)row.x + 1, b); A.src.load(3 * (int)row.x + 2, c);
    float4 rec[3];
    upd::tri_record(a, b, c, rec);
    float4* o = A.tris + 3 * (size_t)j;
    o[0] = rec[0]; o[1] = rec[1]; o[2] = rec[2];
    if (row.y != LeafBihUpdateInfo::kNoPair) {  // emit_pairs: word w of the record is r[6 w ..] = A.x B.x A.y B.y A.z B.z
      float* r = A.tripairs + (size_t)(row.y & (LeafBihUpdateInfo::kPairHalfB - 1u));
      const uint32_t half = (row.y & LeafBihUpdateInfo::kPairHalfB) ? 1u : 0u;
      const bool both = (row.y & LeafBihUpdateInfo::kPairBoth) != 0;
      for (int w = 0; w < 3; w++) {
        const float v[3] = {rec[w].x, rec[w].y, rec[w].z};
        for (int k = 0; k < 3; k++) {
          r[6 * w + 2 * k + half] = v[k];
          if (both) r[6 * w + 2 * k + 1] = v[k];
        }
      }
    }
    float lo[3] = {upd::plane_lo0(), upd::plane_lo0(), upd::plane_lo0()}, hi[3] = {upd::plane_hi0(), upd::plane_hi0(), upd::plane_hi0()};
    upd::plane_add(a, lo, hi); upd::plane_add(b, lo, hi); upd::plane_add(c, lo, hi);
    upd::store_rows(A.ws + 2 * (size_t)j, lo, hi);
  });
}

// A child's plane-form box.  A leaf: the fold of its records' boxes, its count in the reference or, for 7 and more, in its slot with its
// first record (flatten.hpp: BREF_*); an empty leaf keeps the empty box.  A branch: the box the level below it wrote for its slot.
__device__ __forceinline__ void child_box(const DLevelArgs& A, uint32_t ref, float lo[3], float hi[3]) {
  if (ref & BREF_LEAF_BIT) {
    uint32_t count = (ref >> 26) & 7u, first = ref & (BREF_FIRST_LIMIT - 1u);
    if (count == 7u) { const float4 ln = A.bihnodes[first]; count = __float_as_uint(ln.z); first = __float_as_uint(ln.w); }
    for (int a = 0; a < 3; a++) { lo[a] = upd::plane_lo0(); hi[a] = upd::plane_hi0(); }
    upd::fold_rows(A.ws_tri + 2 * (size_t)(first - A.first_rec), 0u, count, 1u, lo, hi);
  } else {
    const float4 l = A.ws_node[2 * (size_t)(ref - A.first_slot)], h = A.ws_node[2 * (size_t)(ref - A.first_slot) + 1];
    lo[0] = l.x; lo[1] = l.y; lo[2] = l.z; hi[0] = h.x; hi[1] = h.y; hi[2] = h.z;
  }
}
// One branch node: its planes into bihnodes and pknodes (.zw, the child references in either form, keep their bits), its box into the
// workspace.  The plane of an empty leaf stays at -inf / +inf (emit_bih: the walk never enters it).
__device__ __forceinline__ void refit_node(const DLevelArgs& A, uint32_t slot) {
  const float4 nd = A.bihnodes[slot];
  const uint32_t z = __float_as_uint(nd.z), lref = z >> 2, rref = __float_as_uint(nd.w);
  const int axis = (int)(z & 3u);
  float llo[3], lhi[3], rlo[3], rhi[3];
  child_box(A, lref, llo, lhi);
  child_box(A, rref, rlo, rhi);
  const float inf = __builtin_huge_valf();
  const float ls = lref == BREF_LEAF_BIT ? -inf : (axis == 0 ? lhi[0] : (axis == 1 ? lhi[1] : lhi[2]));
  const float rs = rref == BREF_LEAF_BIT ? inf : (axis == 0 ? rlo[0] : (axis == 1 ? rlo[1] : rlo[2]));
  A.bihnodes[slot] = make_float4(ls, rs, nd.z, nd.w);
  if (A.pknodes) { const float4 pk = A.pknodes[slot]; A.pknodes[slot] = make_float4(ls, rs, pk.z, pk.w); }
  A.ws_node[2 * (size_t)(slot - A.first_slot)] = make_float4(fminf(llo[0], rlo[0]), fminf(llo[1], rlo[1]), fminf(llo[2], rlo[2]), 0.0f);
  A.ws_node[2 * (size_t)(slot - A.first_slot) + 1] = make_float4(fmaxf(lhi[0], rhi[0]), fmaxf(lhi[1], rhi[1]), fmaxf(lhi[2], rhi[2]), 0.0f);
}

// one level: nodes [first, first + n) of A.nodes
__global__ void __launch_bounds__(64) k_bih_level(DLevelArgs A, uint32_t first, uint32_t n) {
  upd::for_lanes(n, [&](uint32_t j) { refit_node(A, A.nodes[first + j]); });
}
// Levels l0 .. l1 - 1, each of at most kMergeBlock nodes, in one block: level l is A.nodes[off[l] .. off[l + 1]).  Between two levels
// every wave's stores are made visible to the block (a block-scope fence: the block's waves share one CU and its L1, so nothing has to
// be invalidated) and the block meets at its barrier.  The only wait is that barrier.
__global__ void __launch_bounds__(kMergeBlock) k_bih_levels_merged(DLevelArgs A, const uint32_t* off, uint32_t l0, uint32_t l1) {
  for (uint32_t l = l0; l < l1; l++) {
    const uint32_t first = off[l], n = off[l + 1] - first;
    if (threadIdx.x < n) refit_node(A, A.nodes[first + threadIdx.x]);
    __threadfence_block();
    __syncthreads();
  }
}

}  // namespace bihupd
}  // namespace glome
