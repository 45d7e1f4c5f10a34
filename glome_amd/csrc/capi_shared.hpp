// capi_shared.hpp -- what the host half (capi_host.cpp) and the device half (runtime.hip) of the C ABI share: the scene builder's
// handle, what a commit derives from a flattened scene for the choice of kernel instances, and the check of a set of raygen params.
#pragma once
#include <cmath>
#include <string>

#include "../../include/glome_hip.h"
#include "adaptive_rule.hpp"
#include "flatten.hpp"
#include "host_graph.hpp"
#include "instances.hpp"

struct glome_sb {
  glome::Graph graph;
  std::string err;
};
inline const glome::Graph& sb_graph(const glome_sb* sb) { return sb->graph; }

// The commit-time rules in one place: the product's commit (runtime.hip glome_scene_commit), the host's view of them
// (capi_host.cpp glome_sb_scene_traits) and tests/hostsim all take them from here.
struct CommitRules { glome::SceneTraits traits; glome::SceneCaps caps; };
inline CommitRules commit_rules(const glome::Graph& G, const glome::FlatScene& F) {
  CommitRules R;
  R.caps = glome::scene_caps(F);
  glome::SceneTraits& t = R.traits;
  t.tier = (int)F.tier; t.cls_mask = R.caps.cls_mask; t.stack_cap = R.caps.stack_cap; t.pk_all = F.pk_all;
  t.n_bih_nodes = (int64_t)F.bihnodes.size(); t.n_mesh_nodes = (int64_t)F.meshnodes.size() / 4;
  // The flagship render instance and its cull pass take a root entry from the walk-entry table (rt_types.h DScene::walk) and walk it as a triangle
  // bih without looking at its record's kind.  scene_caps gives a void record no class bit, so the class CLS_BIH_TRI alone does not
  // rule one out: an entry of any other kind than a bih keeps the scene off the two-row kernels here (use_two_rows asks for pk_all).
  if (F.tier == 0 && glome::scene_class(t.cls_mask) == glome::CLS_BIH_TRI)
    for (const glome::U4& e : F.entries) if ((F.recs[e.x].x & glome::RF_KINDMASK) != glome::R_BIH) t.pk_all = false;
  for (const glome::Mat& m : G.mats) {
    if (m.kind == glome::MAT_REFLECT || m.kind == glome::MAT_REFRACT || m.kind == glome::MAT_WARP) t.has_secondary_mats = true;
    if (m.kind == glome::MAT_REFRACT) t.has_refract = true;
    if (m.kind == glome::MAT_LAYERS || m.kind == glome::MAT_BLEND) t.has_nested_mats = true;
  }
  return R;
}

// What every lens entry refuses of its raygen params (glome_raygen_count on the host half, the raygen / resolve / render_lens entries on
// the device half): the reason, or null when they are fine.
inline const char* raygen_params_error(const glome_raygen_params* p) {
  if (!p) return "null raygen params";
  if (p->width < 1 || p->height < 1) return "width and height must be at least 1";
  if ((int64_t)p->width * p->height > (1ll << 30)) return "frame too large";
  if (p->samples < 1 || p->samples > glome::kMaxLensSamples) return "samples must be in 1..64";
  if (p->lens != GLOME_LENS_PINHOLE && p->lens != GLOME_LENS_THIN && p->lens != GLOME_LENS_LATLONG) return "unknown lens";
  if (!std::isfinite(p->aperture) || !std::isfinite(p->focus_dist)) return "aperture and focus_dist must be finite";
  if (p->lens == GLOME_LENS_THIN && (p->focus_dist <= 0 || p->aperture < 0)) return "a thin lens needs focus_dist > 0 and aperture >= 0";
  return nullptr;
}
// What the adaptive rule refuses (glome_adaptive_levels / _fold on the host half, glome_render_lens_adaptive on the device half).
inline const char* adaptive_rule_error(int32_t base, int32_t max, float threshold) {
  if (!glome::adaptive::legal(base, max)) return "adaptive levels: base_samples must be even and at least 2, samples = base_samples * 2^k, at most 64";
  if (!(threshold >= 0)) return "the adaptive threshold must be 0 or more (+inf allowed), not NaN";
  return nullptr;
}
