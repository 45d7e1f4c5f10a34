// instance_update_kernels.hpp -- new matrices for committed Instances (glome_scene_instance_update): what flatten.hpp derives from an
// Instance's matrix, made again in the scene's own pools, bit for bit what a commit of the same trees with the new matrices
// (glome_sb_instance_set_transforms) would upload.  Included by runtime.hip only, like the two updates before it, whose plane refit
// (bih_update_kernels.hpp: k_bih_level, refit_node) and bound store (k_bih_bound_store) it launches as they are.
//
// Two things are derived from an Instance's matrix.  Its six float4 in `xfms` are (float) of the 24 doubles (emit, K_INSTANCE: mk4).  And
// a bih that holds the Instance as an item built its planes and its box from the item's box: box_of_points over the eight corners of
// bound(child) through xf_point (host_graph.hpp `bound`, K_INSTANCE), min(p - kDelta) / max(p + kDelta).  A plane is one more pad beyond
// that, rounded outward; the header's box is the items' boxes joined, rounded outward.  Both roundings are monotone, so they commute with
// min and max (the argument of bih_update_kernels.hpp): each corner is rounded to fp32 on its own, in the plane form -- two pads -- and
// in the box form -- one --, and everything above the corners is an fp32 min / max.  xf_point is spelled with explicit round-to-nearest
// multiplications and additions in the host's order, ((m0 x + m1 y) + m2 z) + m3: nothing contracts.
//   k_inst_xfm       one lane per (Instance, slot): the six float4; raises kErrBadVertex for an entry that is not finite
//   k_inst_item_box  one lane per named Instance that is a bih item: its two fp32 boxes into the bih's workspace rows
//   k_inst_box_fold  the box-form rows of all the bih's items folded per wave into partial boxes, for k_bih_bound_store
// The workspace rows persist: the first update of a bih uploads the commit-time rows of all its items (InstBihInfo::rows), later ones
// overwrite the rows of the Instances they name.  The library flushes fp32 subnormals: a component whose fp32 value is subnormal is
// stored as zero, as in the other updates.  No kernel waits for another wave: the order between the launches is the stream's.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "bih_update_kernels.hpp"
#include "flatten.hpp"
#include "mesh_update_kernels.hpp"

namespace glome {
namespace instupd {

struct DXfmArgs {
  const double* xfms;    // 24 per named Instance: forward rows, inverse rows
  const uint2* rows;     // per (Instance, slot): (index into xfms, xfm slot)
  float4* pool;          // the scene's xfms pool
  uint32_t n;            // rows
  unsigned int* error;   // the slot's sticky error word
};
struct DItemArgs {
  const double* xfms;
  const uint2* rows;     // per named Instance that is an item of THIS bih: (index into xfms, item)
  const double* bounds;  // six per item of the bih: bound(child), lo then hi
  const uint32_t* rec_off;  // per item: its record, relative to the tree's first
  float4* ws_plane;      // two per record of the tree's span: the plane-form box
  float4* ws_box;        // two per item: the box-form box
  uint32_t n;            // rows
  unsigned int* error;
};

__global__ void __launch_bounds__(64) k_inst_xfm(DXfmArgs A) {
  const uint32_t items = (A.n + 63u) >> 6;
  for (uint32_t item = blockIdx.x; item < items; item += gridDim.x) {
    const uint32_t j = item * 64u + threadIdx.x;
    if (j >= A.n) continue;
    const uint2 row = A.rows[j];
    const double* m = A.xfms + 24 * (size_t)row.x;
    float4* o = A.pool + 6 * (size_t)row.y;
    bool bad = false;
    for (int q = 0; q < 6; q++) {
      const double a = m[4 * q], b = m[4 * q + 1], c = m[4 * q + 2], d = m[4 * q + 3];
      bad = bad || !(isfinite(a) && isfinite(b) && isfinite(c) && isfinite(d));
      o[q] = make_float4((float)a, (float)b, (float)c, (float)d);
    }
    if (bad) atomicOr(A.error, kErrBadVertex);
  }
}

__global__ void __launch_bounds__(64) k_inst_item_box(DItemArgs A) {
  const uint32_t items = (A.n + 63u) >> 6;
  for (uint32_t item = blockIdx.x; item < items; item += gridDim.x) {
    const uint32_t j = item * 64u + threadIdx.x;
    if (j >= A.n) continue;
    const uint2 row = A.rows[j];
    const double* m = A.xfms + 24 * (size_t)row.x;
    const double* b = A.bounds + 6 * (size_t)row.y;
    const float inf = __builtin_huge_valf();
    float plo[3] = {inf, inf, inf}, phi[3] = {-inf, -inf, -inf}, blo[3] = {inf, inf, inf}, bhi[3] = {-inf, -inf, -inf};
    double dlo[3] = {__builtin_huge_val(), __builtin_huge_val(), __builtin_huge_val()}, dhi[3] = {-__builtin_huge_val(), -__builtin_huge_val(), -__builtin_huge_val()};
    for (int c = 0; c < 8; c++) {
      const double x = b[(c & 4) ? 3 : 0], y = b[(c & 2) ? 4 : 1], z = b[(c & 1) ? 5 : 2];
      double p[3];
      for (int r = 0; r < 3; r++)  // xf_point
        p[r] = __dadd_rn(__dadd_rn(__dadd_rn(__dmul_rn(m[4 * r], x), __dmul_rn(m[4 * r + 1], y)), __dmul_rn(m[4 * r + 2], z)), m[4 * r + 3]);
      bihupd::plane_add(p, plo, phi);
      meshupd::box_add(p, blo, bhi);
      for (int r = 0; r < 3; r++) { dlo[r] = fmin(dlo[r], __dsub_rn(p[r], kDelta)); dhi[r] = fmax(dhi[r], __dadd_rn(p[r], kDelta)); }  // box_of_points, in fp64
    }
    // `bih` refuses a box that reaches the reference's infinity (host_graph.hpp: "bih: infinite bounding box"): the item's folded box, as
    // the host form of the update tests it
    bool huge = false;
    for (int r = 0; r < 3; r++) huge = huge || dlo[r] == -kInfinity || dhi[r] == kInfinity;
    if (huge) atomicOr(A.error, kErrBadVertex);
    float4* wp = A.ws_plane + 2 * (size_t)A.rec_off[row.y];
    wp[0] = make_float4(plo[0], plo[1], plo[2], 0.0f);
    wp[1] = make_float4(phi[0], phi[1], phi[2], 0.0f);
    float4* wb = A.ws_box + 2 * (size_t)row.y;
    wb[0] = make_float4(blo[0], blo[1], blo[2], 0.0f);
    wb[1] = make_float4(bhi[0], bhi[1], bhi[2], 0.0f);
  }
}

// Block b's wave folds the rows b * 64 + lane, (b + gridDim.x) * 64 + lane, ... and stores one partial box: part[2 b ..].  At most
// meshupd::kBoundMaxBlocks blocks, which is what k_bih_bound_store's caller sizes `part` for.
__global__ void __launch_bounds__(64) k_inst_box_fold(const float4* ws_box, uint32_t n, float4* part) {
  const float inf = __builtin_huge_valf();
  float lo[3] = {inf, inf, inf}, hi[3] = {-inf, -inf, -inf};
  for (uint32_t i = blockIdx.x * 64u + threadIdx.x; i < n; i += gridDim.x * 64u) {
    const float4 l = ws_box[2 * (size_t)i], h = ws_box[2 * (size_t)i + 1];
    lo[0] = fminf(lo[0], l.x); lo[1] = fminf(lo[1], l.y); lo[2] = fminf(lo[2], l.z);
    hi[0] = fmaxf(hi[0], h.x); hi[1] = fmaxf(hi[1], h.y); hi[2] = fmaxf(hi[2], h.z);
  }
  meshupd::wave_fold(lo, hi);
  if (threadIdx.x == 0) {
    part[2 * (size_t)blockIdx.x] = make_float4(lo[0], lo[1], lo[2], 0.0f);
    part[2 * (size_t)blockIdx.x + 1] = make_float4(hi[0], hi[1], hi[2], 0.0f);
  }
}

}  // namespace instupd
}  // namespace glome
