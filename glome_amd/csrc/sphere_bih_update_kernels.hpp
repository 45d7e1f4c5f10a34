// sphere_bih_update_kernels.hpp -- new centres and radii for a committed sphere bih (glome_scene_sphere_bih_update): what flatten.hpp's
// emit_bih / emit_prim derive from the items' spheres, made again in the scene's own pools, bit for bit what a commit of the same tree
// with the new spheres (glome_sb_bih_set_spheres) would upload.  Included by runtime.hip only, like bih_update_kernels.hpp, whose level
// pass (k_bih_level, k_bih_levels_merged: refit_node over the workspace rows) it launches as it is, with no packet node copy; the header's
// store is update_common.hpp's k_bound_store, the fp64 bound's fold item_bih_update_kernels.hpp's k_nest_fold_store.
//
// A Sphere's box is c - r / c + r with NO pad (host_graph.hpp `bound`, Sphere.hs:78-81), where a Triangle's carries one kDelta.  So:
//   a branch's planes are round_up(lmax + kDelta) and round_down(rmin - kDelta), lmax / rmin the max / min over a subtree of (c + r)[axis]
//   / (c - r)[axis] from -+kInfinity.  x -> round_up(x + kDelta) and x -> round_down(x - kDelta) are monotone, so they commute with max
//   and min: a record's plane-form box is round_down((c - r) - kDelta) / round_up((c + r) + kDelta), rounded per sphere, and everything
//   above it is an fp32 min / max in any order, from upd::plane_lo0() / plane_hi0() -- what an empty subtree gives on the host;
//   the header's box is round_down / round_up of the join of the c -+ r from box_empty: round_down(c - r) / round_up(c + r) per sphere,
//   folded in fp32 from (float)kInfinity, again by monotonicity;
//   the bih's fp64 bound (what a bih above it is refitted from) is the min / max of the c -+ r themselves from +-kInfinity.
// With r > 0 (both forms of the call require it) c - r and c + r are never -0 in round-to-nearest, so no fold meets a tie between zeros
// of two signs: fp32 and fp64 min / max are exact in any order.  Every c -+ r and -+ kDelta is a __dsub_rn / __dadd_rn in the host's
// order: nothing contracts.  The record is ((float)cx, (float)cy, (float)cz, (float)r), emit_prim's mk4.
//   k_sph_items          one lane per record: the spheres record, its plane-form box into the workspace; raises kErrBadVertex for a value
//                        that is not finite or a radius that is not positive
//   k_sph_bound          a block's partial fp32 box over a strided share of the items, for k_bound_store
//   k_nest_spheres_part  a block's partial fp64 box over a strided share of the items, for k_nest_fold_store
// Each of the three is an instance per sphere source (SphPacked64: fp64 cx cy cz r interleaved; SphSplit32: fp32 centres and radii in two
// streams, glome_scene_sphere_bih_update_f32), one body after the load.
// The library flushes fp32 subnormals: as in the other updates, a component whose fp32 value would be subnormal is stored as zero.
// No kernel waits for another wave: the order between the launches is the stream's.  All stores are ordinary vector stores, each to an
// index below the count its table was sized by, whatever the values.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "bih_update_kernels.hpp"
#include "flatten.hpp"
#include "item_bih_update_kernels.hpp"
#include "update_common.hpp"

namespace glome {
namespace sphupd {

// A sphere source: load(i, s) gives item i as four doubles, cx cy cz r, whatever the caller holds -- the spheres' form of
// update_common.hpp's point source, a template argument of the three kernels that read the input; everything after the load is one body.
//   SphPacked64   c3r[4 i ..], fp64 interleaved: what the update took before there were sources
//   SphSplit32    two fp32 streams, centres [n, 3] and radii [n], as a particle system holds them; fp32 -> fp64 is exact
struct SphPacked64 {
  const double* c3r;
  __device__ __forceinline__ void load(uint32_t i, double s[4]) const { const double* q = c3r + 4 * (size_t)i; s[0] = q[0]; s[1] = q[1]; s[2] = q[2]; s[3] = q[3]; }
};
struct SphSplit32 {
  const float* c;
  const float* r;
  __device__ __forceinline__ void load(uint32_t i, double s[4]) const { const float* q = c + 3 * (size_t)i; s[0] = (double)q[0]; s[1] = (double)q[1]; s[2] = (double)q[2]; s[3] = (double)r[i]; }
};

template <class Src> struct DItemsArgs {
  Src src;               // per item: cx cy cz r
  const uint32_t* rows;  // per record: its item (LeafBihUpdateInfo, one word a row)
  float4* spheres;       // the tree's first record
  float4* ws;            // two per record: the sphere's plane-form box (lo, -) (hi, -), where bihupd::child_box reads it
  uint32_t n;            // records
  unsigned int* error;   // the slot's sticky error word
};

// c - r and c + r of a sphere s = (cx, cy, cz, r), as `bound` makes them
__device__ __forceinline__ void sphere_box(const double s[4], double lo[3], double hi[3]) {
  for (int a = 0; a < 3; a++) { lo[a] = __dsub_rn(s[a], s[3]); hi[a] = __dadd_rn(s[a], s[3]); }
}

template <class Src> __global__ void __launch_bounds__(64) k_sph_items(DItemsArgs<Src> A) {
  upd::for_lanes(A.n, [&](uint32_t j) {
    double s[4];
    A.src.load(A.rows[j], s);
    const double cx = s[0], cy = s[1], cz = s[2], r = s[3];
    if (!(isfinite(cx) && isfinite(cy) && isfinite(cz) && isfinite(r) && r > 0.0)) atomicOr(A.error, kErrBadVertex);
    A.spheres[j] = make_float4((float)cx, (float)cy, (float)cz, (float)r);
    double dlo[3], dhi[3];
    sphere_box(s, dlo, dhi);
    float lo[3], hi[3];
    for (int a = 0; a < 3; a++) {  // the fold of one box from the empty one
      lo[a] = fminf(upd::plane_lo0(), round_down(__dsub_rn(dlo[a], kDelta)));
      hi[a] = fmaxf(upd::plane_hi0(), round_up(__dadd_rn(dhi[a], kDelta)));
    }
    upd::store_rows(A.ws + 2 * (size_t)j, lo, hi);
  });
}

// part[2 b ..]: block b's box over items b * 256 + lane, (b + gridDim.x) * 256 + lane, ..., real infinities where it saw none.  The wave
// folds in registers, the block's four waves through LDS (upd::block_fold32, as k_points_bound does); at most upd::kBoundMaxBlocks blocks.
template <class Src> __global__ void __launch_bounds__(upd::kBoundBlock) k_sph_bound(Src src, uint32_t n, float4* part) {
  __shared__ float sh[upd::kBoundBlock / 64][6];
  const float inf = __builtin_huge_valf();
  float lo[3] = {inf, inf, inf}, hi[3] = {-inf, -inf, -inf};
  for (uint32_t i = blockIdx.x * upd::kBoundBlock + threadIdx.x; i < n; i += gridDim.x * upd::kBoundBlock) {
    double s[4], dlo[3], dhi[3];
    src.load(i, s);
    sphere_box(s, dlo, dhi);
    for (int a = 0; a < 3; a++) { lo[a] = fminf(lo[a], round_down(dlo[a])); hi[a] = fmaxf(hi[a], round_up(dhi[a])); }
  }
  upd::block_fold32(lo, hi, sh);
  if (threadIdx.x == 0) upd::store_rows(part + 2 * (size_t)blockIdx.x, lo, hi);
}

// part[6 b ..]: block b's fp64 box min(c - r) / max(c + r) over its share of the items; at most itemupd::kPartMaxBlocks blocks
template <class Src> __global__ void __launch_bounds__(itemupd::kFoldBlock) k_nest_spheres_part(Src src, uint32_t n, double* part) {
  __shared__ double sh[itemupd::kFoldBlock / 64][6];
  const double inf = __builtin_huge_val();
  double lo[3] = {inf, inf, inf}, hi[3] = {-inf, -inf, -inf};
  for (uint32_t i = blockIdx.x * itemupd::kFoldBlock + threadIdx.x; i < n; i += gridDim.x * itemupd::kFoldBlock) {
    double s[4], dlo[3], dhi[3];
    src.load(i, s);
    sphere_box(s, dlo, dhi);
    for (int a = 0; a < 3; a++) { lo[a] = fmin(lo[a], dlo[a]); hi[a] = fmax(hi[a], dhi[a]); }
  }
  itemupd::block_fold(lo, hi, sh);
  if (threadIdx.x == 0) for (int a = 0; a < 3; a++) { part[6 * (size_t)blockIdx.x + a] = lo[a]; part[6 * (size_t)blockIdx.x + 3 + a] = hi[a]; }
}

}  // namespace sphupd
}  // namespace glome
