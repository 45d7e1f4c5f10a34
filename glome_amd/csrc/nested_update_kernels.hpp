// nested_update_kernels.hpp -- updates of objects that lie under a bih (glome_scene_nested_updates, glome_scene_bih_refit): the bound of a
// moved object on the device in fp64, and the pass that carries it one tree up.  Included by runtime.hip only, like the three updates
// before it, whose plane refit (bih_update_kernels.hpp: k_bih_level), box fold (instance_update_kernels.hpp: k_inst_box_fold) and bound
// store (k_bih_bound_store) it launches as they are.
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
//   k_nest_points_part  a block's partial fp64 box over a strided share of the points, each padded by kDelta
//   k_nest_fold_store   ONE block: folds boxes (partial boxes, or a tree's item boxes) from +-start into an object's row of the bounds
//                       table; raises kErrBadVertex when the box reaches the reference's infinity, as `bih` refuses it
//   k_nest_item_rows    one lane per live item of a tree: its plane-form and box-form fp32 rows and its fp64 box, from the object's bound
//                       (a direct item) or from the bound through the item's matrix in the tree's table (an instanced item)
//   k_nest_inst_named   one lane per named Instance that is an item of the tree: k_inst_item_box's work with the child's bound taken
//                       from the bounds table when the child is live, and the matrix and the fp64 box kept in the tree's tables
// instanced_boxes is k_inst_item_box's arithmetic, operation for operation; that kernel stays as it is (its code object is the parent's).
// No kernel waits for another wave: the order between the launches is the stream's.  All stores are ordinary vector stores.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "bih_update_kernels.hpp"
#include "flatten.hpp"
#include "mesh_update_kernels.hpp"

namespace glome {
namespace nestupd {

constexpr int kFoldBlock = 256, kPartMaxBlocks = 256;
constexpr uint32_t kInstancedBit = 1u << 31, kNoLive = 0xffffffffu;

struct DItemsArgs {
  const uint2* live;        // per live item of the tree: (item, the object's row of `bounds` | kInstancedBit)
  const double* bounds;     // the scene's table: six per live object (lo, hi)
  const double* xf;         // the tree's table: 24 per item (forward rows, inverse rows)
  const uint32_t* rec_off;  // per item: its record, relative to the tree's first
  float4* ws_plane;         // two per record of the tree's span
  float4* ws_box;           // two per item
  double* box64;            // six per item
  uint32_t n;               // live items
  unsigned int* error;      // the slot's sticky error word
};
struct DNamedArgs {
  const double* xfms;        // 24 per named Instance
  const uint2* rows;         // per named Instance that is an item of THIS tree: (index into xfms, item)
  const double* child_bounds;  // six per item: bound(child) at commit
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

// the fold of a block's lanes into lane 0 (valid there alone)
__device__ __forceinline__ void block_fold(double lo[3], double hi[3], double (*sh)[6]) {
  for (int d = 32; d >= 1; d >>= 1)
    for (int a = 0; a < 3; a++) { lo[a] = fmin(lo[a], __shfl_xor(lo[a], d, 64)); hi[a] = fmax(hi[a], __shfl_xor(hi[a], d, 64)); }
  if ((threadIdx.x & 63) == 0) for (int a = 0; a < 3; a++) { sh[threadIdx.x >> 6][a] = lo[a]; sh[threadIdx.x >> 6][3 + a] = hi[a]; }
  __syncthreads();
  if (threadIdx.x == 0)
    for (int w = 1; w < kFoldBlock / 64; w++) for (int a = 0; a < 3; a++) { lo[a] = fmin(lo[a], sh[w][a]); hi[a] = fmax(hi[a], sh[w][3 + a]); }
}

// part[6 b ..]: block b's box over points b * 256 + lane, (b + gridDim.x) * 256 + lane, ...; real infinities where it saw none
__global__ void __launch_bounds__(kFoldBlock) k_nest_points_part(const double* pts, uint32_t n, double* part) {
  __shared__ double sh[kFoldBlock / 64][6];
  const double inf = __builtin_huge_val();
  double lo[3] = {inf, inf, inf}, hi[3] = {-inf, -inf, -inf};
  for (uint32_t i = blockIdx.x * kFoldBlock + threadIdx.x; i < n; i += gridDim.x * kFoldBlock) {
    double p[3];
    meshupd::d3_load(pts, (int)i, p);
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
// k_inst_item_box's arithmetic: xf_point in the host's order, ((m0 x + m1 y) + m2 z) + m3, every corner rounded on its own.
__device__ __forceinline__ void instanced_boxes(const double* m, const double* b, float plo[3], float phi[3], float blo[3], float bhi[3], double dlo[3], double dhi[3]) {
  const float inf = __builtin_huge_valf();
  for (int r = 0; r < 3; r++) { plo[r] = inf; phi[r] = -inf; blo[r] = inf; bhi[r] = -inf; dlo[r] = __builtin_huge_val(); dhi[r] = -__builtin_huge_val(); }
  for (int c = 0; c < 8; c++) {
    const double x = b[(c & 4) ? 3 : 0], y = b[(c & 2) ? 4 : 1], z = b[(c & 1) ? 5 : 2];
    double p[3];
    for (int r = 0; r < 3; r++)  // xf_point
      p[r] = __dadd_rn(__dadd_rn(__dadd_rn(__dmul_rn(m[4 * r], x), __dmul_rn(m[4 * r + 1], y)), __dmul_rn(m[4 * r + 2], z)), m[4 * r + 3]);
    bihupd::plane_add(p, plo, phi);
    meshupd::box_add(p, blo, bhi);
    for (int r = 0; r < 3; r++) { dlo[r] = fmin(dlo[r], __dsub_rn(p[r], kDelta)); dhi[r] = fmax(dhi[r], __dadd_rn(p[r], kDelta)); }
  }
}
// an item's three boxes into the tree's tables; raises the bad-input bit for a box `bih` refuses
__device__ __forceinline__ void store_item(uint32_t item, const uint32_t* rec_off, float4* ws_plane, float4* ws_box, double* box64, unsigned int* error,
                                           const float plo[3], const float phi[3], const float blo[3], const float bhi[3], const double dlo[3], const double dhi[3]) {
  bool huge = false;
  for (int r = 0; r < 3; r++) huge = huge || dlo[r] == -kInfinity || dhi[r] == kInfinity;
  if (huge) atomicOr(error, kErrBadVertex);
  float4* wp = ws_plane + 2 * (size_t)rec_off[item];
  wp[0] = make_float4(plo[0], plo[1], plo[2], 0.0f);
  wp[1] = make_float4(phi[0], phi[1], phi[2], 0.0f);
  float4* wb = ws_box + 2 * (size_t)item;
  wb[0] = make_float4(blo[0], blo[1], blo[2], 0.0f);
  wb[1] = make_float4(bhi[0], bhi[1], bhi[2], 0.0f);
  for (int r = 0; r < 3; r++) { box64[6 * (size_t)item + r] = dlo[r]; box64[6 * (size_t)item + 3 + r] = dhi[r]; }
}

__global__ void __launch_bounds__(64) k_nest_item_rows(DItemsArgs A) {
  const uint32_t items = (A.n + 63u) >> 6;
  for (uint32_t it = blockIdx.x; it < items; it += gridDim.x) {
    const uint32_t j = it * 64u + threadIdx.x;
    if (j >= A.n) continue;
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
    store_item(row.x, A.rec_off, A.ws_plane, A.ws_box, A.box64, A.error, plo, phi, blo, bhi, dlo, dhi);
  }
}

__global__ void __launch_bounds__(64) k_nest_inst_named(DNamedArgs A) {
  const uint32_t items = (A.n + 63u) >> 6;
  for (uint32_t it = blockIdx.x; it < items; it += gridDim.x) {
    const uint32_t j = it * 64u + threadIdx.x;
    if (j >= A.n) continue;
    const uint2 row = A.rows[j];
    const double* m = A.xfms + 24 * (size_t)row.x;
    double* keep = A.xf + 24 * (size_t)row.y;
    for (int q = 0; q < 24; q++) keep[q] = m[q];
    const uint32_t lv = A.item_live[row.y];
    // (no bounds table yet: the switch has never been on, so no object under a bih has moved and the commit's bound is the child's)
    const double* b = (lv == kNoLive || !A.bounds) ? A.child_bounds + 6 * (size_t)row.y : A.bounds + 6 * (size_t)lv;
    float plo[3], phi[3], blo[3], bhi[3];
    double dlo[3], dhi[3];
    instanced_boxes(m, b, plo, phi, blo, bhi, dlo, dhi);
    store_item(row.y, A.rec_off, A.ws_plane, A.ws_box, A.box64, A.error, plo, phi, blo, bhi, dlo, dhi);
  }
}

}  // namespace nestupd
}  // namespace glome
