// instances.hpp -- the table of kernel instances and the rules that choose one for a scene and a set of render params.
// Plain C++17, no HIP types: the host half (capi_host.cpp: glome_kernel_choice), the host runtime (runtime.hip), the kernel parts
// (kernel_parts.hip) and tests/hostsim all include it.
//   X-lists     every flat-tier instance, listed once by the part that compiles it; kernel_parts.hip makes the launchers from them,
//               instance_listed() the compile-time check that the rules below only ever name a listed instance
//   scene_caps  the commit-time rules (entry classes, LDS / overflow stack entries, the generic tier's packet stack)
//   choose_render / choose_sampler / choose_trace   scene traits + params -> Choice (instance key, launch bound, stack rows)
#pragma once
#include <algorithm>
#include <cstring>
#include <utility>

#include "rt_types.h"

namespace glome {

#ifndef GLOME_GENERIC_LB
#define GLOME_GENERIC_LB 2  // waves per SIMD the generic-tier kernels are compiled for (256 VGPRs)
#endif
// ------------------------------------------------------------------------------------------------ kernel instances by part
// Every instance the host runtime can ask for, listed once; the part that holds an instance defines the launcher that knows it.
#ifndef GLOME_CSG_LB
#define GLOME_CSG_LB 2  // waves per SIMD of the (CSG | primitives) instances
#endif
#ifndef GLOME_FLAG_LB
#define GLOME_FLAG_LB 6  // waves per SIMD of the flagship instance (two stack rows, every ray a packet)
#endif
constexpr int render_flat_key(bool F, bool C, bool U, int CLS, int LB, bool TWO) { return (F ? 1 : 0) | (C ? 2 : 0) | (U ? 4 : 0) | (TWO ? 8 : 0) | (LB << 4) | (CLS << 8); }
constexpr int ss_flat_key(bool U, int CLS, int LB, bool TWO, bool F) { return (F ? 1 : 0) | (U ? 4 : 0) | (TWO ? 8 : 0) | (LB << 4) | (CLS << 8); }
// k_render_flat<FAITHFUL, COUNT, FULL, CLS, LB, TWO_ROWS>
#define GLOME_RENDER_FLAT_P1(X) /* production, lean */                                                                      \
  X(false, false, false, CLS_BIH_TRI, 1, false) X(false, false, false, (CLS_BIH_SPHERE | CLS_PRIMS), 1, false) X(false, false, false, CLS_MESH, 1, false) \
  X(false, false, false, CLS_ALL, 1, false) X(false, false, false, CLS_BIH_TRI, GLOME_FLAG_LB, true)
#define GLOME_RENDER_FLAT_P2(X) /* production, full (secondary rays, nested materials) */                                   \
  X(false, false, true, CLS_BIH_TRI, 1, false) X(false, false, true, (CLS_BIH_SPHERE | CLS_PRIMS), 1, false) X(false, false, true, CLS_MESH, 1, false) \
  X(false, false, true, CLS_ALL, 1, false)
#define GLOME_RENDER_FLAT_P3(X) /* the CSG class (two waves per SIMD: S4 0.72 -> 0.52 ms; three spill).  Round 3: an instance of its own for scenes of CSG items and plain primitives only -- 223 / 256 registers with 0 / 17 spills where the every-class one spills 22 / 39: S4 0.455 -> 0.393 ms */                    \
  X(false, false, false, CLS_EVERY, 2, false) X(false, false, true, CLS_EVERY, 2, false)                                     \
  X(false, false, false, (CLS_CSG | CLS_PRIMS), GLOME_CSG_LB, false) X(false, false, true, (CLS_CSG | CLS_PRIMS), GLOME_CSG_LB, false) /* CSG items and plain primitives only (S4) */
#define GLOME_RENDER_FLAT_P4(X) /* faithful / counting */                                                                   \
  X(true, true, true, CLS_EVERY, 1, false) X(true, true, false, CLS_EVERY, 1, false) X(false, true, true, CLS_EVERY, 1, false) X(false, true, false, CLS_EVERY, 1, false)
// k_ss_frame_flat<FULL, CLS, LB, TWO_ROWS, FAITHFUL>
#define GLOME_SS_FLAT_P5(X) X(false, CLS_BIH_TRI, 5, true, false) X(false, CLS_BIH_TRI, 4, true, false) X(false, CLS_BIH_TRI, 1, false, false) X(true, CLS_BIH_TRI, 1, false, false)
#define GLOME_SS_FLAT_P9(X) X(true, CLS_EVERY, 1, false, true) X(false, CLS_EVERY, 2, false, false) X(true, CLS_EVERY, 2, false, false) \
  X(false, (CLS_CSG | CLS_PRIMS), 2, false, false) X(true, (CLS_CSG | CLS_PRIMS), 2, false, false)
// k_trace_batch_flat<FAITHFUL, COUNT, FULL, CLS, LB> (trace_kernels.hpp): what choose_trace can name -- choose_render's instances without the two-row one
#define GLOME_TRACE_FLAT_P12(X) /* production, lean */                                                                      \
  X(false, false, false, CLS_BIH_TRI, 1) X(false, false, false, (CLS_BIH_SPHERE | CLS_PRIMS), 1) X(false, false, false, CLS_MESH, 1) \
  X(false, false, false, CLS_ALL, 1) X(false, false, false, CLS_EVERY, 2) X(false, false, false, (CLS_CSG | CLS_PRIMS), GLOME_CSG_LB)
#define GLOME_TRACE_FLAT_P13(X) /* production, full */                                                                      \
  X(false, false, true, CLS_BIH_TRI, 1) X(false, false, true, (CLS_BIH_SPHERE | CLS_PRIMS), 1) X(false, false, true, CLS_MESH, 1) \
  X(false, false, true, CLS_ALL, 1) X(false, false, true, CLS_EVERY, 2) X(false, false, true, (CLS_CSG | CLS_PRIMS), GLOME_CSG_LB)
#define GLOME_TRACE_FLAT_P14(X) /* faithful / counting */                                                                   \
  X(true, true, true, CLS_EVERY, 1) X(true, true, false, CLS_EVERY, 1) X(false, true, true, CLS_EVERY, 1) X(false, true, false, CLS_EVERY, 1)
// the units of the device half: 0 is runtime.hip, 1..kParts-1 are kernel_parts.hip with -DGLOME_PART=k (glome_amd/build.py reads the count from here)
#define GLOME_NPARTS 16
constexpr int kParts = GLOME_NPARTS;

// is `key` one of the listed instances (the lists the launchers of kernel_parts.hip are made from)
#define GLOME_KEY_OF_RENDER_FLAT(F, C, U, K, B, T) || key == render_flat_key(F, C, U, K, B, T)
#define GLOME_KEY_OF_SS_FLAT(U, K, B, T, F) || key == ss_flat_key(U, K, B, T, F)
#define GLOME_KEY_OF_TRACE_FLAT(F, C, U, K, B) || key == render_flat_key(F, C, U, K, B, false)
enum InstanceKind : int { KIND_RENDER = 0, KIND_SAMPLER = 1, KIND_TRACE = 2 };
constexpr bool instance_listed(InstanceKind kind, int key) {
  if (kind == KIND_TRACE) return false GLOME_TRACE_FLAT_P12(GLOME_KEY_OF_TRACE_FLAT) GLOME_TRACE_FLAT_P13(GLOME_KEY_OF_TRACE_FLAT) GLOME_TRACE_FLAT_P14(GLOME_KEY_OF_TRACE_FLAT);
  return kind == KIND_RENDER
             ? (false GLOME_RENDER_FLAT_P1(GLOME_KEY_OF_RENDER_FLAT) GLOME_RENDER_FLAT_P2(GLOME_KEY_OF_RENDER_FLAT) GLOME_RENDER_FLAT_P3(GLOME_KEY_OF_RENDER_FLAT) GLOME_RENDER_FLAT_P4(GLOME_KEY_OF_RENDER_FLAT))
             : (false GLOME_SS_FLAT_P5(GLOME_KEY_OF_SS_FLAT) GLOME_SS_FLAT_P9(GLOME_KEY_OF_SS_FLAT));
}

// ------------------------------------------------------------------------------------------------ commit-time rules
// what the choice of an instance looks at: made once per scene, at commit (capi_shared.hpp commit_rules)
struct SceneTraits {
  int tier = 1;
  int cls_mask = CLS_ALL;  // which entry classes the flat root program contains
  bool has_secondary_mats = false, has_nested_mats = false;
  bool has_refract = false;  // a Refract material: its transmitted rays are not unit length (Shader.hs:141) -- see exact_traversal
  bool pk_all = false;       // the hand-written walk can take every root entry it would be given: every triangle BIH of the scene has its
                             // node form (flatten.hpp emit_bih) and, in a scene of class CLS_BIH_TRI, every root entry is a bih (commit_rules)
  int stack_cap = 8;         // stack entries per lane in LDS
  int64_t n_bih_nodes = 0, n_mesh_nodes = 0;
};
struct SceneCaps {
  int cls_mask = CLS_ALL;
  int stack_cap = 8, ovf_cap = 0;  // stack entries per lane in LDS, and beyond the LDS part
  uint32_t pk_generic_cap = 0;
};
// FLAT: flatten.hpp's FlatScene (a template so that this header stands without the flattener)
template <class FLAT> SceneCaps scene_caps(const FLAT& F) {
  SceneCaps c;
  // the generic tier's kernels carry an LDS stack of up to kGenericPacketStack entries per lane for the packet walks of its service
  // (sphere / triangle trees, trees of items answered in place: 18 KB a wave at 24, eight waves per CU fit); a deeper tree keeps the
  // per-lane walk
  c.pk_generic_cap = (F.tier != 0 && F.max_sphere_bih_depth > 0) ? (uint32_t)std::min(kGenericPacketStack, std::max(4, F.max_sphere_bih_depth)) : 0u;
  if (F.tier == 0) {
    int m = 0;
    for (const U4& e : F.entries) {
      const U4& r = F.recs[e.x];
      uint32_t k = r.x & RF_KINDMASK;
      if (k == R_BIH) { uint32_t cl; memcpy(&cl, &F.bihhdr[3 * r.y + 1].w, 4); m |= cl == BC_TRI ? CLS_BIH_TRI : (cl == BC_SPHERE ? CLS_BIH_SPHERE : (cl == BC_CSG ? CLS_CSG : CLS_BIH_SIMPLE)); }
      else if (k == R_MESH) m |= CLS_MESH;
      else if (k > R_CONE) m |= CLS_CSG;  // a Difference / Intersection / Instance over primitives in the root list
      else if (k != R_VOID) m |= CLS_PRIMS;
    }
    c.cls_mask = m;
  }
  int need = std::max(F.max_bih_depth, F.max_mesh_depth);
  // LDS holds up to kLdsStack entries per lane (LDS per wave bounds occupancy); a deeper tree keeps its correctness
  // through the global overflow columns.
  constexpr int kLdsStack = kAsmLdsCap;
  int total = std::min(kFlatStack, std::max(4, need));
  if (F.tier == 0 && F.max_mesh_depth > 0) total = std::max(total, std::min(kFlatStackMesh, 2 * F.max_mesh_depth));  // (the Mesh packet walk: up to two entries per level)
  c.stack_cap = std::max(4, std::min(kLdsStack, total));
  c.ovf_cap = std::max(0, total - c.stack_cap);
  return c;
}

// ------------------------------------------------------------------------------------------------ the choice
// generic: the interpreter's kernel (counting bih_nodes / prim_tests or lean); otherwise `key` names a flat-tier instance of the kind asked
// for, compiled for `lb` waves per SIMD and two or three stack rows per entry; faithful: the instance's FAITHFUL argument.
struct Choice { bool generic; bool generic_counts; int key; bool two_rows; int lb; bool faithful; };
// wave slots per CU an instance's register budget allows (what a persistent grid is capped by)
constexpr int waves_per_cu(const Choice& c) { return c.two_rows ? 4 * c.lb : 32; }

constexpr int scene_class(int m) {  // scene class -> the smallest kernel instance that covers it (SPECIALIZE analogue, Bih.hs:370-374)
  if (m & CLS_CSG) return (m & ~(CLS_CSG | CLS_PRIMS)) == 0 ? (CLS_CSG | CLS_PRIMS) : CLS_EVERY;
  return (m & ~CLS_BIH_TRI) == 0 ? CLS_BIH_TRI : ((m & ~(CLS_BIH_SPHERE | CLS_PRIMS)) == 0 ? (CLS_BIH_SPHERE | CLS_PRIMS) : ((m & ~CLS_MESH) == 0 ? CLS_MESH : CLS_ALL));
}
// every ray of the frame is walked as a packet (see k_render_flat): two stack rows per entry, six waves per SIMD
constexpr bool use_two_rows(const SceneTraits& s, bool faithful, bool count_work, int tile_stride, uint32_t items = 0xffffffffu) {
  // a small launch of a rank's shard shares the GPU with the collective's and the blit's kernels and is better off with the
  // 16-wave instance (measured at 8 ranks: 0.040 against 0.047 ms per frame); from ~48k work items on the 24-wave one wins
  if (tile_stride != 1 && items < 48000u) return false;
  if (s.tier != 0 || faithful || count_work) return false;
  if (s.has_secondary_mats || s.has_nested_mats || s.stack_cap != kAsmLdsCap || !s.pk_all) return false;
  return scene_class(s.cls_mask) == CLS_BIH_TRI;  // (what bih_walk_asm walks: a two-row kernel has no row for bih_tri_packet's references)
}
// A scene with a Refract material, traced deeper than the primary ray: the transmitted rays are not unit length
// (Shader.hs:141), and for those rayint_sphere (Sphere.hs:20-41) reports hits outside the sphere's box -- the ordered
// early-out's pruning is exact only for unit rays, so such a frame is traversed as the reference traverses (the flat
// tier's faithful instance; the generic tier switches per ray, rt_generic.hpp).
constexpr bool exact_traversal(bool has_refract, int maxdepth) { return has_refract && maxdepth > 1; }
// lean kernel: legal when no secondary trace can do work and no material nests (Blend / AdditiveLayers)
constexpr bool full_shading(const SceneTraits& s, int maxdepth) { return s.has_nested_mats || (s.has_secondary_mats && maxdepth > 1); }

// renderTile: `items` = the launch's work items (all its frames)
constexpr Choice choose_render(const SceneTraits& s, bool faithful_asked, bool count_work, int maxdepth, int tile_stride, uint32_t items) {
  const bool two_rows = use_two_rows(s, faithful_asked, count_work, tile_stride, items);
  if (s.tier != 0) return Choice{true, count_work, 0, false, GLOME_GENERIC_LB, false};
  const bool faithful = faithful_asked || exact_traversal(s.has_refract, maxdepth), count = count_work || faithful;
  const bool full = full_shading(s, maxdepth);
  if (two_rows) return Choice{false, false, render_flat_key(false, false, false, CLS_BIH_TRI, GLOME_FLAG_LB, true), true, GLOME_FLAG_LB, false};
  if (faithful) return Choice{false, false, render_flat_key(true, true, full, CLS_EVERY, 1, false), false, 1, true};
  if (count) return Choice{false, false, render_flat_key(false, true, full, CLS_EVERY, 1, false), false, 1, false};
  const int cls = scene_class(s.cls_mask), lb = cls == CLS_EVERY ? 2 : (cls == (CLS_CSG | CLS_PRIMS) ? GLOME_CSG_LB : 1);
  return Choice{false, false, render_flat_key(false, false, full, cls, lb, false), false, lb, false};
}
// renderTileSubsample.  The sampler has a triangle-class instance only (no Mesh or sphere class), and its two-row rule never looks at the item count.
constexpr Choice choose_sampler(const SceneTraits& s, bool faithful_asked, bool count_work, int maxdepth, int tile_stride) {
  const bool two_rows = use_two_rows(s, faithful_asked, count_work, tile_stride) && scene_class(s.cls_mask) == CLS_BIH_TRI;
  if (s.tier != 0) return Choice{true, count_work, 0, false, GLOME_GENERIC_LB, false};
  const bool full = full_shading(s, maxdepth);
  const bool tri = (s.cls_mask & ~CLS_BIH_TRI) == 0;
  const bool refr = exact_traversal(s.has_refract, maxdepth);
  // (four waves per SIMD: with 80 registers the sampler's own state spills, and every reload waits for the loads in flight;
  // a tree of a million nodes misses the caches often enough that a fifth wave pays for the spills of 96 registers:
  // S5 2.28 -> 2.12 ms per frame, S3 0.294 -> 0.310)
  const int lb2 = s.n_bih_nodes > 500000 ? 5 : 4;
  if (two_rows) return Choice{false, false, ss_flat_key(false, CLS_BIH_TRI, lb2, true, false), true, lb2, false};
  if (tri && !full) return Choice{false, false, ss_flat_key(false, CLS_BIH_TRI, 1, false, false), false, 1, false};
  if (tri && !refr) return Choice{false, false, ss_flat_key(true, CLS_BIH_TRI, 1, false, false), false, 1, false};
  // (a Refract material traced deeper than the primary ray: the reference's own traversal, see exact_traversal)
  if (full && refr) return Choice{false, false, ss_flat_key(true, CLS_EVERY, 1, false, true), false, 1, true};
  return Choice{false, false, ss_flat_key(full, scene_class(s.cls_mask) == (CLS_CSG | CLS_PRIMS) ? (CLS_CSG | CLS_PRIMS) : CLS_EVERY, 2, false, false), false, 2, false};
}
// Trace.trace over a caller's ray streams (trace_kernels.hpp): choose_render's rule without the two-row instance, which is tied to the
// frame's item loop (item table, coordinate tables) and to rays that are all packets -- a caller's rays need not be.
constexpr Choice choose_trace(const SceneTraits& s, bool faithful_asked, bool count_work, int maxdepth) {
  if (s.tier != 0) return Choice{true, count_work, 0, false, GLOME_GENERIC_LB, false};
  const bool faithful = faithful_asked || exact_traversal(s.has_refract, maxdepth), count = count_work || faithful;
  const bool full = full_shading(s, maxdepth);
  if (faithful) return Choice{false, false, render_flat_key(true, true, full, CLS_EVERY, 1, false), false, 1, true};
  if (count) return Choice{false, false, render_flat_key(false, true, full, CLS_EVERY, 1, false), false, 1, false};
  const int cls = scene_class(s.cls_mask), lb = cls == CLS_EVERY ? 2 : (cls == (CLS_CSG | CLS_PRIMS) ? GLOME_CSG_LB : 1);
  return Choice{false, false, render_flat_key(false, false, full, cls, lb, false), false, lb, false};
}

// ------------------------------------------------------------------------------------------------ soundness, at compile time
// Every combination of the inputs the rules look at (the value grid of tests/test_kernel_choice.py), one (tier, cls_mask) slice per
// constant evaluation: each choice that is not the interpreter's names a listed instance, so a launcher that answers "no kernel
// instance" can only come from a broken build.
constexpr bool choices_listed(int tier, int cls_mask) {
  for (int flags = 0; flags < 16; flags++)
    for (int sc = 0; sc < 2; sc++)
      for (int p = 0; p < 64; p++) {
        SceneTraits s;
        s.tier = tier; s.cls_mask = cls_mask;
        s.has_secondary_mats = flags & 1; s.has_nested_mats = flags & 2; s.has_refract = flags & 4; s.pk_all = flags & 8;
        s.stack_cap = sc ? kAsmLdsCap : (kAsmLdsCap == 8 ? 4 : 8);
        const bool faithful = p & 1, count_work = p & 2;
        const int maxdepth = (p & 4) ? 2 : 1, tile_stride = (p & 8) ? 8 : 1;
        const uint32_t items = (p & 16) ? 48000u : 47999u;
        s.n_bih_nodes = (p & 32) ? 500001 : 500000;
        const Choice r = choose_render(s, faithful, count_work, maxdepth, tile_stride, items);
        const Choice a = choose_sampler(s, faithful, count_work, maxdepth, tile_stride);
        if (!r.generic && !instance_listed(KIND_RENDER, r.key)) return false;
        if (!a.generic && !instance_listed(KIND_SAMPLER, a.key)) return false;
        if (p < 8) {  // (the trace rule looks at faithful, count_work and maxdepth only)
          const Choice t = choose_trace(s, faithful, count_work, maxdepth);
          if (!t.generic && !instance_listed(KIND_TRACE, t.key)) return false;
        }
      }
  return true;
}
template <int I> struct ChoiceSlice { static constexpr bool ok = choices_listed(I & 1, I >> 1); };
template <int... I> constexpr bool all_choices_listed(std::integer_sequence<int, I...>) { return (ChoiceSlice<I>::ok && ...); }
// (asserted once, in capi_host.cpp: the sweep takes a compiler ten seconds and more)

}  // namespace glome
