// item_bih_update_kernels.hpp -- the updates of an item bih, a bih that holds Instances, Meshes or Bihs as items: new matrices for
// committed Instances (glome_scene_instance_update), and updates of objects that lie under a bih (glome_scene_nested_updates,
// glome_scene_bih_refit): the bound of a moved object on the device in fp64, and the pass that carries it one tree up.  What flatten.hpp
// derives from an Instance's matrix and from its items' bounds is made again in the scene's own pools, bit for bit what a commit of the
// same trees with the new matrices (glome_sb_instance_set_transforms) and the moved objects would upload.  Included by runtime.hip only,
// like the two updates before it, whose plane refit (bih_update_kernels.hpp: k_bih_level, refit_node) and bound store
// (update_common.hpp: k_bound_store) it launches as they are.
//
// Two things are derived from an Instance's matrix.  Its six float4 in `xfms` are (float) of the 24 doubles (emit, K_INSTANCE: mk4).  And
// a bih that holds the Instance as an item built its planes and its box from the item's box: box_of_points over the eight corners of
// bound(child) through xf_point (host_graph.hpp `bound`, K_INSTANCE), min(p - kDelta) / max(p + kDelta).  A plane is one more pad beyond
// that, rounded outward; the header's box is the items' boxes joined, rounded outward.  Both roundings are monotone, so they commute with
// min and max (the argument of bih_update_kernels.hpp): each corner is rounded to fp32 on its own, in the plane form -- two pads -- and
// in the box form -- one --, and everything above the corners is an fp32 min / max.  xf_point is spelled with explicit round-to-nearest
// multiplications and additions in the host's order, ((m0 x + m1 y) + m2 z) + m3: nothing contracts.
//
// A bih built its planes and its box from bound(item) of its items (host_graph.hpp `bih`, Graph::bih_refit).  For an item that is a Mesh
// or a Bih under wrappers that is the object's own fp64 box; for an Instance of one, box_of_points over the eight corners of that box
// through xf_point.  The object's box is itself a fold: a Mesh's box_of_points over all vertices (from a vertex: the fold starts at real
// infinities), a triangle bih's the join of its triangles' boxes from box_empty (+-kInfinity = 1e6), an item bih's the join of its items'
// boxes from box_empty.  fp64 min / max of finite values is exact in any order, so a grid-stride fold, shuffles across the wave and LDS
// across the block give the host's value to the bit.  Every p - kDelta / p + kDelta is a __dsub_rn / __dadd_rn: nothing contracts.  A
// sum p -+ kDelta that is zero is +0 (round to nearest), and a fold whose operands tie at zero keeps +0 whenever one of them is +0
// (fmin / fmax of +0 and -0 may return either: -0 arises only from a matrix product, and only a tie with it could show); the stored sign
// is the fold's, and the tests keep their coordinates away from it.
//   k_inst_xfm          one lane per (Instance, slot): the six float4; raises kErrBadVertex for an entry that is not finite
//   k_xfm_convert       one lane per named Instance: its 24 doubles from a matrix source (XfmSrc: a pair, a forward matrix or a pose,
//                       fp64 or fp32, strided, after a base matrix or not) into the scene's table, which the two kernels around it
//                       in this list then read as they read a caller's fp64 array (glome_scene_instance_update_from)
//   k_nest_inst_named   one lane per named Instance that is an item of the tree: its two fp32 boxes into the tree's workspace rows; as
//                       <true>, with the child's bound taken from the bounds table when the child is live, and the matrix and the
//                       fp64 box kept in the tree's tables (<false>: a tree without live items while the switch is off)
//   k_nest_item_rows    one lane per live item of a tree: its plane-form and box-form fp32 rows and its fp64 box, from the object's bound
//                       (a direct item) or from the bound through the item's matrix in the tree's table (an instanced item)
//   k_inst_box_fold     the box-form rows of all the tree's items folded per wave into partial boxes, for k_bound_store
//   k_nest_points_part  a block's partial fp64 box over a strided share of the points, each padded by kDelta
//   k_nest_fold_store   ONE block: folds boxes (partial boxes, or a tree's item boxes) from +-start into an object's row of the bounds
//                       table; raises kErrBadVertex when the box reaches the reference's infinity, as `bih` refuses it
// The workspace rows persist: the first update or refit of a tree uploads the commit-time rows of all its items (InstBihInfo::rows), later
// ones overwrite the rows of the Instances they name and of the live items.  The library flushes fp32 subnormals: a component whose fp32
// value is subnormal is stored as zero, as in the other updates.
// No kernel waits for another wave: the order between the launches is the stream's.  All stores are ordinary vector stores.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "bih_update_kernels.hpp"
#include "flatten.hpp"
#include "update_common.hpp"
#include "xfm_sources.hpp"

namespace glome {
namespace itemupd {

constexpr int kFoldBlock = 256, kPartMaxBlocks = 256;
constexpr uint32_t kInstancedBit = 1u << 31, kNoLive = 0xffffffffu;

struct DXfmArgs {
  const double* xfms;    // 24 per named Instance: forward rows, inverse rows
  const uint2* rows;     // per (Instance, slot): (index into xfms, xfm slot)
  float4* pool;          // the scene's xfms pool
  uint32_t n;            // rows
  unsigned int* error;   // the slot's sticky error word
};
struct DItemsArgs {
  const uint2* live;        // per live item of the tree: (item, the object's row of `bounds` | kInstancedBit)
  const double* bounds;     // the scene's table: six per live object (lo, hi)
  const double* xf;         // the tree's table: 24 per item (forward rows, inverse rows)
  const uint32_t* rec_off;  // per item: its record, relative to the tree's first
  float4* ws_plane;         // two per record of the tree's span: the plane-form box
  float4* ws_box;           // two per item: the box-form box
  double* box64;            // six per item
  uint32_t n;               // live items
  unsigned int* error;      // the slot's sticky error word
};
struct DNamedArgs {
  const double* xfms;        // 24 per named Instance
  const uint2* rows;         // per named Instance that is an item of THIS tree: (index into xfms, item)
  const double* child_bounds;  // six per item: bound(child) at commit, lo then hi
  const uint32_t* item_live;   // per item: the child's row of `bounds`, kNoLive when the child is static
  const double* bounds;        // null until the switch has been on once
  double* xf;
  const uint32_t* rec_off;
  float4* ws_plane;
  float4* ws_box;
  double* box64;
  uint32_t n;
  unsigned int* error;
};

__global__ void __launch_bounds__(64) k_inst_xfm(DXfmArgs A) {
  upd::for_lanes(A.n, [&](uint32_t j) {
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
  });
}

// A matrix source: load(k, m) gives the matrix of the k-th named Instance as 24 doubles, whatever the caller holds -- the point sources
// of update_common.hpp, for matrices.  Item k is the width_of(FORM) values of T from data + k * stride (stride in elements, at least the
// width: the index is 64-bit, and nothing outside the item is read, so what lies between two items may be anything); xfm::convert
// (xfm_sources.hpp, the host functions' own body) makes the 24 doubles of them, and with a base the result is xfm::mult(item, base[k]):
// the item applied after the base.  fp32 -> fp64 is exact, so an fp32 source gives what the fp64 source gives for the widened array.
// False for what the POSE form refuses (a quaternion of length 0, s <= 0).
template <class T, int FORM> struct XfmSrc {
  const T* data;
  const double* base;  // null, or 24 doubles per item, contiguous
  int64_t stride;
  __device__ __forceinline__ bool load(uint32_t k, double m[24]) const {
    constexpr int W = FORM == xfm::kPair ? 24 : FORM == xfm::kForward ? 12 : 8;
    const T* p = data + (int64_t)k * stride;
    double v[W];
    for (int q = 0; q < W; q++) v[q] = (double)p[q];
    if (!base) return xfm::convert(FORM, v, m);
    double item[24], b[24];
    const bool ok = xfm::convert(FORM, v, item);
    for (int q = 0; q < 24; q++) b[q] = base[24 * (size_t)k + q];
    xfm::mult(item, b, m);
    return ok;
  }
};
template <class Src> struct DConvertArgs {
  Src src;
  double* table;         // 24 per named Instance: what k_inst_xfm and k_nest_inst_named read as `xfms`
  uint32_t n;            // named Instances
  unsigned int* error;   // the slot's sticky error word
};
// Raises kErrBadVertex for a lane whose source refuses its item or whose 24 results are not all finite (an input that is not finite, a
// singular forward matrix: 0 / 0 and x / 0 are not finite); the row is stored all the same, and the readers raise the bit again.
template <class Src> __global__ void __launch_bounds__(64) k_xfm_convert(DConvertArgs<Src> A) {
  upd::for_lanes(A.n, [&](uint32_t k) {
    double m[24];
    bool bad = !A.src.load(k, m);
    double* o = A.table + 24 * (size_t)k;
    for (int q = 0; q < 24; q++) { bad = bad || !isfinite(m[q]); o[q] = m[q]; }
    if (bad) atomicOr(A.error, kErrBadVertex);
  });
}

// Block b's wave folds the rows b * 64 + lane, (b + gridDim.x) * 64 + lane, ... and stores one partial box: part[2 b ..].  At most
// upd::kBoundMaxBlocks blocks, which is what k_bound_store's caller sizes `part` for.
__global__ void __launch_bounds__(64) k_inst_box_fold(const float4* ws_box, uint32_t n, float4* part) {
  const float inf = __builtin_huge_valf();
  float lo[3] = {inf, inf, inf}, hi[3] = {-inf, -inf, -inf};
  upd::fold_rows(ws_box, blockIdx.x * 64u + threadIdx.x, n, gridDim.x * 64u, lo, hi);
  upd::wave_fold(lo, hi);
  if (threadIdx.x == 0) upd::store_rows(part + 2 * (size_t)blockIdx.x, lo, hi);
}

// the fold of a block's lanes into lane 0 (valid there alone)
__device__ __forceinline__ void block_fold(double lo[3], double hi[3], double (*sh)[6]) {
  for (int d = 32; d >= 1; d >>= 1)
    for (int a = 0; a < 3; a++) { lo[a] = fmin(lo[a], __shfl_xor(lo[a], d, 64)); hi[a] = fmax(hi[a], __shfl_xor(hi[a], d, 64)); }
  if ((threadIdx.x & 63) == 0) for (int a = 0; a < 3; a++) { sh[threadIdx.x >> 6][a] = lo[a]; sh[threadIdx.x >> 6][3 + a] = hi[a]; }
  __syncthreads();
  if (threadIdx.x == 0)
    for (int w = 1; w < kFoldBlock / 64; w++) for (int a = 0; a < 3; a++) { lo[a] = fmin(lo[a], sh[w][a]); hi[a] = fmax(hi[a], sh[w][3 + a]); }
}

// part[6 b ..]: block b's box over points b * 256 + lane, (b + gridDim.x) * 256 + lane, ... of a point source (update_common.hpp); real
// infinities where it saw none
template <class Src> __global__ void __launch_bounds__(kFoldBlock) k_nest_points_part(Src pts, uint32_t n, double* part) {
  __shared__ double sh[kFoldBlock / 64][6];
  const double inf = __builtin_huge_val();
  double lo[3] = {inf, inf, inf}, hi[3] = {-inf, -inf, -inf};
  for (uint32_t i = blockIdx.x * kFoldBlock + threadIdx.x; i < n; i += gridDim.x * kFoldBlock) {
    double p[3];
    pts.load((int)i, p);
    for (int a = 0; a < 3; a++) { lo[a] = fmin(lo[a], __dsub_rn(p[a], kDelta)); hi[a] = fmax(hi[a], __dadd_rn(p[a], kDelta)); }
  }
  block_fold(lo, hi, sh);
  if (threadIdx.x == 0) for (int a = 0; a < 3; a++) { part[6 * (size_t)blockIdx.x + a] = lo[a]; part[6 * (size_t)blockIdx.x + 3 + a] = hi[a]; }
}

// one block: boxes[6 i ..], i < n, folded from (start, -start) into out6
__global__ void __launch_bounds__(kFoldBlock) k_nest_fold_store(const double* boxes, uint32_t n, double start, double* out6, unsigned int* error) {
  __shared__ double sh[kFoldBlock / 64][6];
  double lo[3] = {start, start, start}, hi[3] = {-start, -start, -start};
  for (uint32_t i = threadIdx.x; i < n; i += kFoldBlock)
    for (int a = 0; a < 3; a++) { lo[a] = fmin(lo[a], boxes[6 * (size_t)i + a]); hi[a] = fmax(hi[a], boxes[6 * (size_t)i + 3 + a]); }
  block_fold(lo, hi, sh);
  if (threadIdx.x == 0) {
    bool huge = false;
    for (int a = 0; a < 3; a++) { out6[a] = lo[a]; out6[3 + a] = hi[a]; huge = huge || lo[a] == -kInfinity || hi[a] == kInfinity; }
    if (huge) atomicOr(error, kErrBadVertex);
  }
}

// An Instance item's boxes from its matrix m (24) and its child's bound b (6): the plane form, the box form, and box_of_points in fp64.
// xf_point in the host's order, ((m0 x + m1 y) + m2 z) + m3, every corner rounded on its own.
__device__ __forceinline__ void instanced_boxes(const double* m, const double* b, float plo[3], float phi[3], float blo[3], float bhi[3], double dlo[3], double dhi[3]) {
  const float inf = __builtin_huge_valf();
  for (int r = 0; r < 3; r++) { plo[r] = inf; phi[r] = -inf; blo[r] = inf; bhi[r] = -inf; dlo[r] = __builtin_huge_val(); dhi[r] = -__builtin_huge_val(); }
  for (int c = 0; c < 8; c++) {
    const double x = b[(c & 4) ? 3 : 0], y = b[(c & 2) ? 4 : 1], z = b[(c & 1) ? 5 : 2];
    double p[3];
    for (int r = 0; r < 3; r++)  // xf_point
      p[r] = __dadd_rn(__dadd_rn(__dadd_rn(__dmul_rn(m[4 * r], x), __dmul_rn(m[4 * r + 1], y)), __dmul_rn(m[4 * r + 2], z)), m[4 * r + 3]);
    upd::plane_add(p, plo, phi);
    upd::box_add(p, blo, bhi);
    for (int r = 0; r < 3; r++) { dlo[r] = fmin(dlo[r], __dsub_rn(p[r], kDelta)); dhi[r] = fmax(dhi[r], __dadd_rn(p[r], kDelta)); }  // box_of_points, in fp64
  }
}
// An item's three boxes into the tree's tables.  `bih` refuses a box that reaches the reference's infinity (host_graph.hpp: "bih: infinite
// bounding box"): the item's folded fp64 box, as the host form of the update tests it, raises the bad-input bit.  KEEP_TABLES: the fp64
// box goes into the tree's box64 row too.
template <bool KEEP_TABLES>
__device__ __forceinline__ void store_item(uint32_t item, const uint32_t* rec_off, float4* ws_plane, float4* ws_box, double* box64, unsigned int* error,
                                           const float plo[3], const float phi[3], const float blo[3], const float bhi[3], const double dlo[3], const double dhi[3]) {
  bool huge = false;
  for (int r = 0; r < 3; r++) huge = huge || dlo[r] == -kInfinity || dhi[r] == kInfinity;
  if (huge) atomicOr(error, kErrBadVertex);
  upd::store_rows(ws_plane + 2 * (size_t)rec_off[item], plo, phi);
  upd::store_rows(ws_box + 2 * (size_t)item, blo, bhi);
  if (KEEP_TABLES) for (int r = 0; r < 3; r++) { box64[6 * (size_t)item + r] = dlo[r]; box64[6 * (size_t)item + 3 + r] = dhi[r]; }
}

__global__ void __launch_bounds__(64) k_nest_item_rows(DItemsArgs A) {
  upd::for_lanes(A.n, [&](uint32_t j) {
    const uint2 row = A.live[j];
    const double* b = A.bounds + 6 * (size_t)(row.y & ~kInstancedBit);
    float plo[3], phi[3], blo[3], bhi[3];
    double dlo[3], dhi[3];
    if (row.y & kInstancedBit) instanced_boxes(A.xf + 24 * (size_t)row.x, b, plo, phi, blo, bhi, dlo, dhi);
    else  // bound(item) is the object's: flatten.hpp emit_bih's rows of it
      for (int r = 0; r < 3; r++) {
        dlo[r] = b[r]; dhi[r] = b[3 + r];
        plo[r] = round_down(__dsub_rn(dlo[r], kDelta)); phi[r] = round_up(__dadd_rn(dhi[r], kDelta));
        blo[r] = round_down(dlo[r]); bhi[r] = round_up(dhi[r]);
      }
    store_item<true>(row.x, A.rec_off, A.ws_plane, A.ws_box, A.box64, A.error, plo, phi, blo, bhi, dlo, dhi);
  });
}

// The kernel of an Instance update's named items: instanced_boxes + store_item, one kernel in two instances.
//  - KEEP_TABLES (a tree with live items, switch on or off, and any tree while the switch is on): the matrix and the fp64 box go into
//    the tree's xf / box64 rows, and a live child's bound comes from the bounds table.  A child that is not live (item_live[item] ==
//    kNoLive), or any child while there is no bounds table, takes child_bounds, the commit's bound(child): the switch has never been
//    on, or the child cannot move, so that is the child's bound as it stands.
//  - !KEEP_TABLES (a tree without live items while the switch is off): child_bounds and the two fp32 rows, nothing else -- what
//    k_inst_item_box was.  Such a tree has no live child (item_live is kNoLive throughout), so this is the other instance's arithmetic
//    on the other instance's operands; and nothing reads its xf / box64 rows while the switch is off (only k_nest_item_rows, which has
//    no live item to run for here, and the tree's fp64 fold, which the host launches with the switch on alone), so no answer depends
//    on the two stores.  The KEEP_TABLES instance would serve here too, and did in a measurement: the oak's Instance update (2,047 and
//    16 named items, switch off) took 0.1074 and 0.0846 ms where this form takes 0.1038 and 0.0816, 3.6 % beyond a run-to-run spread
//    of 1.5 % (profiles/update_refactor_rate.txt).  So the plain form stays, as an instance rather than a copy.
template <bool KEEP_TABLES> __global__ void __launch_bounds__(64) k_nest_inst_named(DNamedArgs A) {
  upd::for_lanes(A.n, [&](uint32_t j) {
    const uint2 row = A.rows[j];
    const double* m = A.xfms + 24 * (size_t)row.x;
    if (KEEP_TABLES) {
      double* keep = A.xf + 24 * (size_t)row.y;
      for (int q = 0; q < 24; q++) keep[q] = m[q];
    }
    const uint32_t lv = KEEP_TABLES ? A.item_live[row.y] : kNoLive;
    // (no bounds table yet: the switch has never been on, so no object under a bih has moved and the commit's bound is the child's)
    const double* b = (lv == kNoLive || !A.bounds) ? A.child_bounds + 6 * (size_t)row.y : A.bounds + 6 * (size_t)lv;
    float plo[3], phi[3], blo[3], bhi[3];
    double dlo[3], dhi[3];
    instanced_boxes(m, b, plo, phi, blo, bhi, dlo, dhi);
    store_item<KEEP_TABLES>(row.y, A.rec_off, A.ws_plane, A.ws_box, A.box64, A.error, plo, phi, blo, bhi, dlo, dhi);
  });
}

}  // namespace itemupd
}  // namespace glome
