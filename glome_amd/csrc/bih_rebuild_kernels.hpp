// bih_rebuild_kernels.hpp -- the first step of a re-split of a committed triangle or sphere bih (glome_scene_bih_rebuild,
// glome_scene_sphere_bih_rebuild; runtime.hip): the items' fp64 boxes as the host builder's `bound` makes them, straight from an update's
// source (update_common.hpp, sphere_bih_update_kernels.hpp), in the layout the device builder's level loop reads (bih_build_device.hpp).
// Included by runtime.hip only.
//
// A triangle's box is min(p) - delta / max(p) + delta per axis with Graph::bound's own selects (gmin(gmin(p1, p2), p3): a > b ? b : a)
// and one round-to-nearest subtraction / addition; a sphere's is c - r / c + r.  The same pass joins the boxes into the root's -- atomics
// on the builder's order-preserving keys, which give the host's fold but for the sign of a zero (bih_build_device.hpp says why that
// reaches neither the tree nor a status) -- and validates every value: one that is not finite, a radius that is not positive or a vertex
// index outside [0, nv) raises `flag`, a word of the call's own and not the slot's sticky error word, so that a refused rebuild leaves
// no trace in the context.  A bad index is clamped BEFORE the load, as in the update: nothing is read out of bounds.
#pragma once
#include <hip/hip_runtime.h>

#include "bih_build_device.hpp"
#include "sphere_bih_update_kernels.hpp"
#include "update_common.hpp"

namespace glome {
namespace bihrebuild {

enum : unsigned int { kBadValue = 1u, kBadIndex = 2u };  // the bits of `flag`

// point k of a source, with the call's own flag for an index out of range (IndexedPts::load would raise the slot's word)
template <class T> __device__ __forceinline__ void point_of(const upd::DensePts<T>& s, uint32_t k, double v[3], unsigned int& bad) { (void)bad; s.load((int)k, v); }
template <class T> __device__ __forceinline__ void point_of(const upd::IndexedPts<T>& s, uint32_t k, double v[3], unsigned int& bad) {
  uint32_t i = (uint32_t)s.idx[(size_t)k];
  if (i >= s.nv) { bad |= kBadIndex; i = 0u; }  // (a negative index is a large unsigned one)
  v[0] = (double)s.p[3 * (size_t)i]; v[1] = (double)s.p[3 * (size_t)i + 1]; v[2] = (double)s.p[3 * (size_t)i + 2];
}
__device__ __forceinline__ double d_gmin(double a, double b) { return a > b ? b : a; }  // gmin / gmax, host_graph.hpp
__device__ __forceinline__ double d_gmax(double a, double b) { return a > b ? a : b; }

// item i's box; SPHERE: the source yields spheres, else the item's three points
template <class Src, bool SPHERE> __device__ __forceinline__ void item_box(const Src& src, uint32_t i, double lo[3], double hi[3], unsigned int& bad) {
  if constexpr (SPHERE) {
    double s[4];
    src.load(i, s);
    if (!(isfinite(s[0]) && isfinite(s[1]) && isfinite(s[2]) && isfinite(s[3]) && s[3] > 0.0)) bad |= kBadValue;
    sphupd::sphere_box(s, lo, hi);
  } else {
    double p[3][3];
    for (uint32_t c = 0; c < 3; c++) {
      point_of(src, 3u * i + c, p[c], bad);
      if (!(isfinite(p[c][0]) && isfinite(p[c][1]) && isfinite(p[c][2]))) bad |= kBadValue;
    }
    for (int a = 0; a < 3; a++) {
      lo[a] = __dsub_rn(d_gmin(d_gmin(p[0][a], p[1][a]), p[2][a]), kDelta);
      hi[a] = __dadd_rn(d_gmax(d_gmax(p[0][a], p[1][a]), p[2][a]), kDelta);
    }
  }
}

// box: 6 n doubles, SoA (bihdev::levels_dev); root: six keys, lo then hi, preset to the keys of box_empty; flag: preset to 0
template <class Src, bool SPHERE> __global__ void __launch_bounds__(256) k_item_boxes(Src src, uint32_t n, double* box, unsigned long long* root, unsigned int* flag) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  unsigned int bad = 0;
  unsigned long long klo[3], khi[3];
  for (int a = 0; a < 3; a++) { klo[a] = bihdev::dkey(kInfinity); khi[a] = bihdev::dkey(-kInfinity); }
  if (i < n) {
    double lo[3], hi[3];
    item_box<Src, SPHERE>(src, i, lo, hi, bad);
    for (int a = 0; a < 3; a++) {
      box[(size_t)a * n + i] = lo[a]; box[(size_t)(3 + a) * n + i] = hi[a];
      klo[a] = bihdev::dkey(lo[a]); khi[a] = bihdev::dkey(hi[a]);
    }
  }
  // the wave's join and its flags, then one set of atomics per wave
  for (int d = 32; d >= 1; d >>= 1) {
    bad |= (unsigned int)__shfl_xor((int)bad, d, 64);
    for (int a = 0; a < 3; a++) {
      const unsigned long long x = (unsigned long long)__shfl_xor((long long)klo[a], d, 64), y = (unsigned long long)__shfl_xor((long long)khi[a], d, 64);
      klo[a] = x < klo[a] ? x : klo[a];
      khi[a] = y > khi[a] ? y : khi[a];
    }
  }
  if ((threadIdx.x & 63u) == 0u) {
    for (int a = 0; a < 3; a++) { atomicMin(&root[a], klo[a]); atomicMax(&root[3 + a], khi[a]); }
    if (bad) atomicOr(flag, bad);
  }
}

// the root's six bounds back from their keys, beside the flag: what the host reads before the first level
__global__ void k_root_box(const unsigned long long* root, double* out6) {
  if (threadIdx.x < 6) out6[threadIdx.x] = bihdev::dunkey(root[threadIdx.x]);
}

}  // namespace bihrebuild
}  // namespace glome
