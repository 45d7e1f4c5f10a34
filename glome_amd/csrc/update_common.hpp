// update_common.hpp -- the device pieces the scene updates share (mesh_update_kernels.hpp, bih_update_kernels.hpp,
// item_bih_update_kernels.hpp): a point folded into an fp32 box in its two forms, a triangle's record, the fold of stored boxes, the
// loop of a one-lane-per-element kernel, and the fp32 bound of a point array.  Included by runtime.hip only, through those headers.
//
// Every fp32 value an update stores is a (float) rounding of an fp64 expression, or round_down / round_up (flatten.hpp) of a min / max of
// padded fp64 values.  The roundings are monotone, so they commute with min and max: a point is rounded to fp32 on its own and everything
// above it is an fp32 min / max, exact in any order (p -+ kDelta is never -0, so there is no tie between zeros of two signs either).
// Each header argues this for the values it makes.  fp64 arithmetic is spelled with explicit round-to-nearest operations in the host's
// expression order (host_graph.hpp: operator-, cross, normalize): nothing contracts.
//   for_lanes        the grid-stride loop over 64-element items, one lane per element
//   DensePts / IndexedPts   where an update reads its points: a point source yields point k as three doubles, whatever the caller holds
//   fold_rows        stored boxes -- float4 row pairs (lo, -) (hi, -) -- folded into lo / hi
//   block_fold32     a block's boxes folded into lane 0: the shared tail of k_points_bound and sphupd::k_sph_bound
//   k_points_bound   the box over ALL points of an array (Mesh.hs:55), per block, and the check that every coordinate is finite
//   k_bound_store    folds the blocks' boxes, from a start value, into a header's two box words
// No kernel waits for another wave: the order between the launches is the stream's.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "flatten.hpp"

namespace glome {
namespace upd {

// Grid-stride over 64-element items, like k_camera_rays: f(j) for every element j < n the block's lane owns.
template <class F> __device__ __forceinline__ void for_lanes(uint32_t n, F f) {
  const uint32_t items = (n + 63u) >> 6;
  for (uint32_t item = blockIdx.x; item < items; item += gridDim.x) {
    const uint32_t j = item * 64u + threadIdx.x;
    if (j < n) f(j);
  }
}

// A point source: load(k, v) gives point k of an update's input as three doubles.  The kernels that read the input take the source as a
// template argument -- an instance per kind rather than a copy per kind -- and everything after the load is the one body on the same
// doubles: fp32 -> fp64 is exact, so an fp32 source gives what the fp64 source gives for the widened array, bit for bit (a subnormal
// fp32 input may be read as zero: the library flushes them).
//   DensePts<T>     point k is p[3 k ..], T = double (what every update took before there were sources: that instance's loads are
//                   the ones it had) or float
//   IndexedPts<T>   point k is p[3 idx[k] ..]: a vertex array and an index table, as a simulation holds a mesh.  An index outside
//                   [0, nv) ORs kErrBadVertex into the slot's error word and reads vertex 0 instead: the index is clamped BEFORE the
//                   load, so nothing is read out of bounds whatever the table holds (the host refuses nv == 0 with points to read).
template <class T> struct DensePts {
  const T* p;
  __device__ __forceinline__ void load(int k, double v[3]) const { v[0] = (double)p[3 * (size_t)k]; v[1] = (double)p[3 * (size_t)k + 1]; v[2] = (double)p[3 * (size_t)k + 2]; }
};
template <class T> struct IndexedPts {
  const T* p;
  const int32_t* idx;
  uint32_t nv;
  unsigned int* error;   // the slot's sticky error word
  __device__ __forceinline__ void load(int k, double v[3]) const {
    uint32_t i = (uint32_t)idx[(size_t)k];
    if (i >= nv) { atomicOr(error, kErrBadVertex); i = 0u; }  // (a negative index is a large unsigned one)
    v[0] = (double)p[3 * (size_t)i]; v[1] = (double)p[3 * (size_t)i + 1]; v[2] = (double)p[3 * (size_t)i + 2];
  }
};
// a vertex folded into an fp32 box: lo = round_down(p - kDelta), hi = round_up(p + kDelta) (box_of_points' pad, flatten.hpp's roundings)
__device__ __forceinline__ void box_add(const double p[3], float lo[3], float hi[3]) {
  for (int a = 0; a < 3; a++) { lo[a] = fminf(lo[a], round_down(__dsub_rn(p[a], kDelta))); hi[a] = fmaxf(hi[a], round_up(__dadd_rn(p[a], kDelta))); }
}

// where a plane-form fold starts: what an empty subtree gives on the host (bih_update_kernels.hpp)
__device__ __forceinline__ float plane_lo0() { return round_down(__dsub_rn(kInfinity, kDelta)); }
__device__ __forceinline__ float plane_hi0() { return round_up(__dadd_rn(-kInfinity, kDelta)); }
// a vertex folded into a plane-form box: the item's pad and the plane's, two fp64 additions (not p -+ 2 kDelta), rounded outward once
__device__ __forceinline__ void plane_add(const double p[3], float lo[3], float hi[3]) {
  for (int k = 0; k < 3; k++) {
    lo[k] = fminf(lo[k], round_down(__dsub_rn(__dsub_rn(p[k], kDelta), kDelta)));
    hi[k] = fmaxf(hi[k], round_up(__dadd_rn(__dadd_rn(p[k], kDelta), kDelta)));
  }
}

// A triangle's record (p1, n.x) (e1, n.y) (e2, n.z) from its vertices: emit_mesh's and emit_tri's expression (flatten.hpp), in the host's
// order, rounded once.  The Mesh's records and the triangle bih's.
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

// The boxes rows[2 i], rows[2 i + 1] -- (lo, -) (hi, -) -- for i = first, first + step, ... below n, folded into lo / hi, which the caller
// has started: a leaf's records one after another, or a wave's / a grid's strided share of a table.
__device__ __forceinline__ void fold_rows(const float4* rows, uint32_t first, uint32_t n, uint32_t step, float lo[3], float hi[3]) {
  for (uint32_t i = first; i < n; i += step) {
    const float4 l = rows[2 * (size_t)i], h = rows[2 * (size_t)i + 1];
    lo[0] = fminf(lo[0], l.x); lo[1] = fminf(lo[1], l.y); lo[2] = fminf(lo[2], l.z);
    hi[0] = fmaxf(hi[0], h.x); hi[1] = fmaxf(hi[1], h.y); hi[2] = fmaxf(hi[2], h.z);
  }
}
__device__ __forceinline__ void wave_fold(float lo[3], float hi[3]) {
  for (int d = 32; d >= 1; d >>= 1)
    for (int a = 0; a < 3; a++) { lo[a] = fminf(lo[a], __shfl_xor(lo[a], d, 64)); hi[a] = fmaxf(hi[a], __shfl_xor(hi[a], d, 64)); }
}
// a box as a row pair; the .w words are the caller's
__device__ __forceinline__ void store_rows(float4* rows, const float lo[3], const float hi[3], float w0 = 0.0f, float w1 = 0.0f) {
  rows[0] = make_float4(lo[0], lo[1], lo[2], w0);
  rows[1] = make_float4(hi[0], hi[1], hi[2], w1);
}

// The fold of a block of kBoundBlock lanes into lane 0 (valid there alone): across each wave in registers, across the waves through LDS
// (item_bih_update_kernels.hpp block_fold is its fp64 twin).
constexpr int kBoundBlock = 256, kBoundMaxBlocks = 1024;
__device__ __forceinline__ void block_fold32(float lo[3], float hi[3], float (*sh)[6]) {
  wave_fold(lo, hi);
  if ((threadIdx.x & 63) == 0) for (int a = 0; a < 3; a++) { sh[threadIdx.x >> 6][a] = lo[a]; sh[threadIdx.x >> 6][3 + a] = hi[a]; }
  __syncthreads();
  if (threadIdx.x == 0)
    for (int w = 1; w < kBoundBlock / 64; w++) for (int a = 0; a < 3; a++) { lo[a] = fminf(lo[a], sh[w][a]); hi[a] = fmaxf(hi[a], sh[w][3 + a]); }
}

template <class Src> struct DBoundArgs {
  Src src;               // the points
  uint32_t nv;           // how many
  float4* part;          // two per block: (lo, -) (hi, -)
  unsigned int* error;   // the slot's sticky error word
};

// The box over all points of a source -- a Mesh's vertices, unreferenced ones included; a triangle bih's 3 n item vertices (gathered
// through the index table when the source is indexed: a vertex no item references is never read).  A block of 256
// lanes strides over the points, folds across each wave in registers and across its four waves through LDS, and stores one partial box;
// k_bound_store folds the partial boxes.  A lane that meets a coordinate that is not finite ORs kErrBadVertex into the slot's error word
// (glome_ctx_synchronize reports it).
template <class Src> __global__ void __launch_bounds__(kBoundBlock) k_points_bound(DBoundArgs<Src> A) {
  __shared__ float sh[kBoundBlock / 64][6];
  const float inf = __builtin_huge_valf();
  float lo[3] = {inf, inf, inf}, hi[3] = {-inf, -inf, -inf};
  bool bad = false;
  for (uint32_t i = blockIdx.x * kBoundBlock + threadIdx.x; i < A.nv; i += gridDim.x * kBoundBlock) {
    double p[3];
    A.src.load((int)i, p);
    bad = bad || !(isfinite(p[0]) && isfinite(p[1]) && isfinite(p[2]));
    box_add(p, lo, hi);
  }
  if (bad) atomicOr(A.error, kErrBadVertex);
  block_fold32(lo, hi, sh);
  if (threadIdx.x == 0) store_rows(A.part + 2 * (size_t)blockIdx.x, lo, hi);
}
// One wave: the partial boxes, folded from (start, -start), into a header's two box words; .w (the root reference; the unused word or the
// class) keeps its bits.  Where the fold starts shows in a tree of no items or of coordinates beyond 1e6.  A mesh's box is
// box_of_points, which starts from a vertex: its start is real infinity.  A bih's box is a join of item boxes from box_empty
// (host_graph.hpp `bih`): its start is (float)kInfinity, +-kInfinity = 1e6.
__global__ void __launch_bounds__(64) k_bound_store(const float4* part, uint32_t nparts, float start, float4* hdr) {
  float lo[3] = {start, start, start}, hi[3] = {-start, -start, -start};
  fold_rows(part, threadIdx.x, nparts, 64u, lo, hi);
  wave_fold(lo, hi);
  if (threadIdx.x == 0) store_rows(hdr, lo, hi, hdr[0].w, hdr[1].w);
}

}  // namespace upd
}  // namespace glome
