// hostsim.cpp -- TEST INFRASTRUCTURE ONLY.  Compiles the per-ray device headers (rt_device.hpp / rt_generic.hpp)
// as plain host C++ so their logic -- and the flattened layout they index -- can be checked against the oracle on a
// machine without a GPU, before a kernel is ever launched.  It is not part of libglome_hip.so, nothing in glome_amd
// imports it, and bench.py never times it.  GPU parity tests (-m gpu) go through the real C ABI.
#include <cstring>
#include <set>

#include <cstdlib>
#include "host_shim.hpp"  // first: GD / GHD, the one-lane wave, LaneStack -- then the device headers compile for the host
#include "../../glome_amd/csrc/capi_shared.hpp"
#include "../../glome_amd/csrc/flatten.hpp"
#include "../../glome_amd/csrc/rt_device.hpp"
#include "../../glome_amd/csrc/rt_generic.hpp"

using namespace glome;

struct SimScene {
  FlatScene F;
  DScene D;
  CommitRules rules;  // what the product's commit derives for the choice of a kernel instance (capi_shared.hpp)
  std::string err;
};

template <bool FAITHFUL, bool COUNT, bool FULL_> struct HostFlatTier {
  static constexpr bool FULL = FULL_;
  static constexpr bool WARP = false;
  const DScene& S;
  const DLight* lights;
  int nlights;
  LaneStack stk;
  Cnt cnt;
  unsigned int err = 0;
  HitG closest(const Ray& r, float tmax) { HitG ch; Cand c = closest_flat<FAITHFUL, COUNT, CLS_EVERY>(S, r, tmax, stk, cnt, true, &ch, &err); return finalize_flat<CLS_EVERY>(S, r, c, &ch); }
  bool occluded(const Ray& r, float d, uint32_t = 0) { return occluded_flat<COUNT, CLS_EVERY>(S, r, d, stk, cnt, true, &err); }
  // on the host a wave is one lane: the packet code runs as a single-ray traversal
  HitG closest_wave(const Ray& r, float tmax, bool valid, uint32_t = 0) { HitG ch; Cand c = closest_flat<FAITHFUL, COUNT, CLS_EVERY, true>(S, r, tmax, stk, cnt, valid, &ch, &err); return valid ? finalize_flat<CLS_EVERY>(S, r, c, &ch) : hit_miss(); }
  bool occluded_wave(const Ray& r, float d, bool valid) { return occluded_flat<COUNT, CLS_EVERY, true>(S, r, d, stk, cnt, valid, &err); }
};
struct HostStack {
  // a deliberately small "LDS" part so the overflow columns are exercised by the CPU suite too
  static constexpr int LDS_PART = 6;
  uint32_t node[kFlatStack]; float nearv[kFlatStack], farv[kFlatStack];
  uint32_t ovf[3 * kFlatStack];
  LaneStack lane(int cap) {
    LaneStack s; s.node = node; s.nearv = nearv; s.farv = farv; s.cap = LDS_PART < cap ? LDS_PART : cap;
    s.ovf = ovf; s.ovf_cap = cap - s.cap;
    return s;
  }
};
struct HostGenericTier {
  static constexpr bool FULL = true;
  static constexpr bool WARP = true;
  const DScene& S;
  const DLight* lights;
  int nlights;
  Cnt cnt;
  unsigned int err = 0;
  uint32_t vm[kVmWords];
  HostStack pkmem;
  LaneStack pk;  // the packet stack of vm_run's packet service (cap 0: none); packets(): after construction
  void packets() { pk = pkmem.lane((int)S.pk_generic_cap); if (S.pk_generic_cap == 0) { pk.cap = 0; pk.ovf_cap = 0; } }
  HitG closest(const Ray& r, float tmax, uint32_t root) { return vm_closest<true>(S, cnt, err, vm, pk.cap > 0 ? &pk : (LaneStack*)nullptr, r, tmax, root); }
  bool occluded(const Ray& r, float d, uint32_t root) { return vm_occluded<true>(S, cnt, err, vm, pk.cap > 0 ? &pk : (LaneStack*)nullptr, r, d, root); }
  HitG closest(const Ray& r, float tmax) { return closest(r, tmax, S.root_rec); }
  bool occluded(const Ray& r, float d) { return occluded(r, d, S.root_rec); }
  HitG closest_wave(const Ray& r, float tmax, bool valid, uint32_t root) { return valid ? closest(r, tmax, root) : hit_miss(); }
  bool occluded_wave(const Ray& r, float d, bool valid) { return valid && occluded(r, d); }
};

// HostGenericTier with its frame memory outside it: the caller's words (hostsim_frame_probe), so that what the interpreter writes can be read
struct ProbeGenericTier {
  static constexpr bool FULL = true;
  static constexpr bool WARP = true;
  const DScene& S;
  const DLight* lights;
  int nlights;
  Cnt cnt;
  uint32_t* vm;
  unsigned int err = 0;
  HostStack pkmem;
  LaneStack pk;
  void packets() { pk = pkmem.lane((int)S.pk_generic_cap); if (S.pk_generic_cap == 0) { pk.cap = 0; pk.ovf_cap = 0; } }
  HitG closest(const Ray& r, float tmax, uint32_t root) { return vm_closest<true>(S, cnt, err, vm, pk.cap > 0 ? &pk : (LaneStack*)nullptr, r, tmax, root); }
  bool occluded(const Ray& r, float d, uint32_t root) { return vm_occluded<true>(S, cnt, err, vm, pk.cap > 0 ? &pk : (LaneStack*)nullptr, r, d, root); }
  HitG closest(const Ray& r, float tmax) { return closest(r, tmax, S.root_rec); }
  bool occluded(const Ray& r, float d) { return occluded(r, d, S.root_rec); }
  HitG closest_wave(const Ray& r, float tmax, bool valid, uint32_t root) { return valid ? closest(r, tmax, root) : hit_miss(); }
  bool occluded_wave(const Ray& r, float d, bool valid) { return valid && occluded(r, d); }
};


// has the scene a Refract material?  (What the product's rule of the faithful instance asks: instances.hpp exact_traversal, used below.)
static bool refract_scene(const SimScene* s) {
  for (uint32_t k = 0; k < s->D.n_mats; k++) { uint32_t kind; memcpy(&kind, &s->D.mats[3 * k].x, 4); if (kind == DM_REFRACT) return true; }
  return false;
}

extern "C" {
void* hostsim_commit(glome_sb* sb, int root, char* errbuf, int cap) {
  SimScene* s = new SimScene();
  try {
    Flattener fl(sb_graph(sb), s->F);
    fl.run(root);
  } catch (std::exception& e) { snprintf(errbuf, cap, "%s", e.what()); delete s; return nullptr; }
  FlatScene& F = s->F;
  DScene& D = s->D;
  D.recs = F.recs.data(); D.spheres = F.spheres.data(); D.tris = F.tris.data(); D.tripairs = F.tripairs.data(); D.trinorms = F.trinorms.data(); D.boxes = F.boxes.data();
  D.planes = F.planes.data(); D.discs = F.discs.data(); D.quadrics = F.quadrics.data(); D.xfms = F.xfms.data(); D.bihhdr = F.bihhdr.data();
  D.bihnodes = F.bihnodes.data(); D.pknodes = F.pknodes.data(); D.pknodes_bytes = (uint32_t)(F.pknodes.size() * sizeof(F4)); D.meshhdr = F.meshhdr.data(); D.meshnodes = F.meshnodes.data(); D.mtris = F.mtris.data();
  D.mtrimeta = F.mtrimeta.data(); D.mats = F.mats.data(); D.wlights = F.wlights.data(); D.matkids = F.matkids.data(); D.entries = F.entries.data();
  D.n_entries = F.tier == 0 ? (uint32_t)F.entries.size() : 0; D.root_rec = F.root_rec; D.tier = F.tier; D.n_mats = (uint32_t)sb_graph(sb).mats.size(); D.tex_bits = F.tex_bits;
  D.pk_generic_cap = scene_caps(F).pk_generic_cap;  // (the product's commit-time rule, instances.hpp)
  if (getenv("GLOME_DEBUG_NO_GENERIC_PACKETS")) D.pk_generic_cap = 0;  // (the product's switch, runtime.hip glome_scene_commit)
  s->rules = commit_rules(sb_graph(sb), F);
  return s;
}
void hostsim_free(void* s) { delete (SimScene*)s; }
int hostsim_info(void* sv, int* out) {  // tier, nesting, max_bih_depth, max_mesh_depth, n_entries, n_recs
  SimScene* s = (SimScene*)sv;
  out[0] = (int)s->F.tier; out[1] = s->F.nesting_depth; out[2] = s->F.max_bih_depth; out[3] = s->F.max_mesh_depth;
  out[4] = (int)s->D.n_entries; out[5] = (int)s->F.recs.size();
  return 0;
}
// the frame words commit estimated for a ray of this scene (FlatScene::vm_words: what Flattener::run held against kVmWords), and kVmWords
int hostsim_vm_words(void* sv, int* limit) { if (limit) *limit = kVmWords; return ((SimScene*)sv)->F.vm_words; }
// the frame sizes the estimate and the interpreter share (rt_types.h), in the order of helpers.VM_CONSTS
void hostsim_vm_consts(int* out) {
  const int c[] = {kVmWords, kVmHitWords, kVmListR, kVmInstR, kVmBoundR, kVmIbR, kVmDiffFixed, kVmIsectWords, kVmBihFixedR, kVmBihFixedS, kVmIsectChain, kCsgMaxAdvance};
  for (size_t k = 0; k < sizeof(c) / sizeof(c[0]); k++) out[k] = c[k];
}
// The generic tier's interpreter over the caller's rays with its frame memory inside a larger buffer: kVmWords words, then kProbeCanary more
// that nothing may touch.  Every ray runs twice, the buffer filled with one sentinel and then with another; per ray:
//   words[i]   one more than the index of the last frame word that differs from the sentinel, the larger of the two runs -- a LOWER bound of
//              the interpreter's stack height (a frame reserves words it may never write; a word written with the sentinel's own value shows
//              in the other run)
//   flag[i]    the error flag (what the kernels OR into the context's error word)
//   canary[i]  1: the words after kVmWords - 1 are untouched in both runs
//   ans[i]     route 0 rayint: the depth (-1 a miss); 1 shadow: 0 / 1; 2 inside (ox, oy, oz the point): 0 / 1; 3 trace (lights, maxdepth): the depth
// The answer is the second run's; both runs must agree in it and in the flag, or -6 is returned (the frame memory's old contents were read).
int hostsim_frame_probe(void* sv, int route, size_t n, const float* ox, const float* oy, const float* oz, const float* dx, const float* dy, const float* dz,
                        const float* tmax, const float* lights, int nl, int maxdepth, int* words, unsigned char* flag, unsigned char* canary, float* ans) {
  SimScene* s = (SimScene*)sv;
  constexpr int kProbeCanary = 64;
  if (route < 0 || route > 3) return -5;
  if (route == 3 && (nl < 0 || nl > kMaxLights || maxdepth < 1 || maxdepth > kMaxTraceDepth)) return -5;
  DLight L[kMaxLights];
  if (route == 3) for (int i = 0; i < nl; i++) { memcpy(L[i].pos, lights + 8 * i, 12); memcpy(L[i].color, lights + 8 * i + 3, 12); L[i].rad = lights[8 * i + 6]; L[i].shadow = lights[8 * i + 7] != 0; }
  std::vector<uint32_t> buf(kVmWords + kProbeCanary);
  const uint32_t sentinels[2] = {0xa5a5a5a5u, 0x5a5a5a5au};
  for (size_t i = 0; i < n; i++) {
    Ray r; r.o = v3(ox[i], oy[i], oz[i]);
    if (route != 2) r.d = v3(dx[i], dy[i], dz[i]); else r.d = v3(0, 0, 1);
    words[i] = 0; canary[i] = 1;
    float a2[2] = {0, 0}; unsigned int e2[2] = {0, 0};
    for (int k = 0; k < 2; k++) {
      std::fill(buf.begin(), buf.end(), sentinels[k]);
      ProbeGenericTier T{s->D, L, route == 3 ? nl : 0, Cnt(), buf.data()}; T.packets();
      if (route == 0) { HitG h = T.closest(r, tmax[i]); a2[k] = h.hit ? h.t : -1.0f; }
      else if (route == 1) a2[k] = T.occluded(r, tmax[i]) ? 1.0f : 0.0f;
      else if (route == 2) a2[k] = vm_inside(s->D, T.err, buf.data(), 0, s->D.recs[s->D.root_rec], r.o) ? 1.0f : 0.0f;
      else { HitG h; trace_primary(T, r, tmax[i], maxdepth, true, &h); a2[k] = h.hit ? h.t : kInf; }
      e2[k] = T.err;
      int top = kVmWords;
      while (top > 0 && buf[top - 1] == sentinels[k]) top--;
      if (top > words[i]) words[i] = top;
      for (int c = 0; c < kProbeCanary; c++) if (buf[kVmWords + c] != sentinels[k]) canary[i] = 0;
    }
    if (memcmp(&a2[0], &a2[1], 4) != 0 || e2[0] != e2[1]) return -6;
    flag[i] = e2[1] ? 1 : 0; ans[i] = a2[1];
  }
  return 0;
}
// tier: -1 = the scene's own tier, 0 = flat (must be legal), 1 = generic; analysis: faithful traversal + counters
int hostsim_rayint(void* sv, int tier, int analysis, size_t n, const float* ox, const float* oy, const float* oz, const float* dx, const float* dy,
                   const float* dz, const float* tmax, float* t, int* prim, float* nrm, int* tex8, unsigned long long* counters) {
  SimScene* s = (SimScene*)sv;
  if (tier < 0) tier = (int)s->D.tier;
  if (tier == 0 && s->D.tier != 0) return -1;
  HostStack hs;
  Cnt total;
  unsigned int err = 0;
  for (size_t i = 0; i < n; i++) {
    Ray r; r.o = v3(ox[i], oy[i], oz[i]); r.d = v3(dx[i], dy[i], dz[i]);
    HitG h;
    if (tier == 0) {
      if (analysis & 1) { HostFlatTier<true, true, false> T{s->D, nullptr, 0, hs.lane(kFlatStack), Cnt()}; h = (analysis & 2) ? T.closest_wave(r, tmax[i], true) : T.closest(r, tmax[i]); err |= T.err; total.bih += T.cnt.bih; total.prim += T.cnt.prim; total.mesh += T.cnt.mesh; }
      else if (!unit_length(r.d)) { HostFlatTier<true, false, false> T{s->D, nullptr, 0, hs.lane(kFlatStack), Cnt()}; h = T.closest(r, tmax[i]); err |= T.err; }  // (k_rayint_batch_flat's rule for a caller's non-unit ray)
      else { HostFlatTier<false, false, false> T{s->D, nullptr, 0, hs.lane(kFlatStack), Cnt()}; h = (analysis & 2) ? T.closest_wave(r, tmax[i], true) : T.closest(r, tmax[i]); err |= T.err; }  // (k_rayint_batch_flat: `if (T.err)`)
    } else {
      HostGenericTier T{s->D, nullptr, 0, Cnt()}; T.packets();
      h = T.closest(r, tmax[i]);
      err |= T.err; total.bih += T.cnt.bih; total.prim += T.cnt.prim; total.mesh += T.cnt.mesh;
    }
    t[i] = h.hit ? h.t : -1.0f;
    if (prim) prim[i] = h.hit ? (int)h.uid : -1;
    if (nrm) { nrm[3 * i] = h.n.x; nrm[3 * i + 1] = h.n.y; nrm[3 * i + 2] = h.n.z; }
    if (tex8) for (int k = 0; k < 8; k++) tex8[8 * i + k] = (h.hit && k * (int)s->D.tex_bits < 64) ? (int)((h.tex >> (s->D.tex_bits * k)) & ((1ull << s->D.tex_bits) - 1)) - 1 : -1;
  }
  if (counters) { counters[0] = total.bih; counters[1] = total.mesh; counters[2] = total.prim; }
  return err ? -2 : 0;
}
int hostsim_shadow(void* sv, int tier, size_t n, const float* ox, const float* oy, const float* oz, const float* dx, const float* dy, const float* dz,
                   const float* tmax, unsigned char* occ) {
  SimScene* s = (SimScene*)sv;
  if (tier < 0) tier = (int)s->D.tier;
  if (tier == 0 && s->D.tier != 0) return -1;
  HostStack hs;
  unsigned int err = 0;
  for (size_t i = 0; i < n; i++) {
    Ray r; r.o = v3(ox[i], oy[i], oz[i]); r.d = v3(dx[i], dy[i], dz[i]);
    if (tier == 0) { HostFlatTier<false, false, false> T{s->D, nullptr, 0, hs.lane(kFlatStack), Cnt()}; occ[i] = T.occluded(r, tmax[i]); err |= T.err; }
    else { HostGenericTier T{s->D, nullptr, 0, Cnt()}; T.packets(); occ[i] = T.occluded(r, tmax[i]); err |= T.err; }
  }
  return err ? -2 : 0;
}
int hostsim_inside(void* sv, size_t n, const float* px, const float* py, const float* pz, unsigned char* in) {
  SimScene* s = (SimScene*)sv;
  unsigned int err = 0;
  uint32_t vm[kVmWords];
  for (size_t i = 0; i < n; i++) in[i] = vm_inside(s->D, err, vm, 0, s->D.recs[s->D.root_rec], v3(px[i], py[i], pz[i]));
  return err ? -2 : 0;
}
// whole-frame, 1 ray per pixel (renderTile); cam = 12 floats, lights = nl x 8 floats (pos3 col3 rad shadow)
int hostsim_render(void* sv, int tier, const float* cam, const float* lights, int nl, int width, int height, int maxdepth, float* out5, unsigned long long* counters) {
  SimScene* s = (SimScene*)sv;
  if (tier < 0) tier = (int)s->D.tier;
  if (tier == 0 && s->D.tier != 0) return -1;
  DCamera C; memcpy(&C, cam, sizeof(C));
  DLight L[kMaxLights];
  for (int i = 0; i < nl; i++) { memcpy(L[i].pos, lights + 8 * i, 12); memcpy(L[i].color, lights + 8 * i + 3, 12); L[i].rad = lights[8 * i + 6]; L[i].shadow = lights[8 * i + 7] != 0; }
  HostStack hs;
  Cnt total;
  unsigned int err = 0;
  const bool exact = exact_traversal(refract_scene(s), maxdepth);
  for (int py = 0; py < height; py++)
    for (int px = 0; px < width; px++) {
      float xc, yc;
      get_coordsf(width, height, (float)px, (float)py, xc, yc);
      Ray ray = primary_ray(C, xc, yc);
      HitG h; CA c;
      if (tier == 0 && exact) { HostFlatTier<true, false, true> T{s->D, L, nl, hs.lane(kFlatStack), Cnt()}; c = trace_primary(T, ray, kInf, maxdepth, true, &h); err |= T.err; total.shadow += T.cnt.shadow; total.secondary += T.cnt.secondary; }
      else if (tier == 0) { HostFlatTier<false, false, true> T{s->D, L, nl, hs.lane(kFlatStack), Cnt()}; c = trace_primary(T, ray, kInf, maxdepth, true, &h); err |= T.err; total.shadow += T.cnt.shadow; total.secondary += T.cnt.secondary; }
      else { HostGenericTier T{s->D, L, nl, Cnt()}; T.packets(); c = trace_primary(T, ray, kInf, maxdepth, true, &h); err |= T.err; total.shadow += T.cnt.shadow; total.secondary += T.cnt.secondary; }
      float* o = out5 + ((size_t)py * width + px) * 5;
      o[0] = c.r; o[1] = c.g; o[2] = c.b; o[3] = c.a; o[4] = h.hit ? h.t : kInf;
    }
  if (counters) { counters[0] = (unsigned long long)width * height; counters[1] = total.shadow; counters[2] = total.secondary; }
  return err ? -2 : 0;
}

// Trace.trace over a caller's rays (what k_trace_batch_* runs per lane): out5 = (r, g, b, a, depth) per ray, counts = the shadow and the
// secondary rays each ray spawned (words 3 and 4 of a work record).  full = 0 instantiates the tier with FULL == false, so trace_primary
// takes shade_hit_lean; it is refused (-3) where the product's own rule (instances.hpp choose_trace: full_shading) launches no lean kernel
// -- the generic tier has none at all.  faithful: asked for; the rule adds exact_traversal as choose_trace does.
}  // extern "C"
template <class TIER> static void trace_one(TIER& T, const Ray& r, float tmax, int maxdepth, float* o, unsigned int* cnt2, unsigned int& err) {
  HitG h;
  CA c = trace_primary(T, r, tmax, maxdepth, true, &h);
  o[0] = c.r; o[1] = c.g; o[2] = c.b; o[3] = c.a; o[4] = h.hit ? h.t : kInf;
  cnt2[0] = (unsigned int)T.cnt.shadow; cnt2[1] = (unsigned int)T.cnt.secondary;
  err |= T.err;
}
extern "C" {
int hostsim_trace(void* sv, int tier, int full, int faithful, size_t n, const float* ox, const float* oy, const float* oz, const float* dx, const float* dy,
                  const float* dz, const float* tmax, const float* lights, int nl, int maxdepth, float* out5, unsigned int* counts2) {
  SimScene* s = (SimScene*)sv;
  if (tier < 0) tier = (int)s->D.tier;
  if (tier == 0 && s->D.tier != 0) return -1;
  if (nl < 0 || nl > kMaxLights || maxdepth < 1 || maxdepth > kMaxTraceDepth) return -5;
  if (!full && (tier != 0 || full_shading(s->rules.traits, maxdepth))) return -3;
  DLight L[kMaxLights];
  for (int i = 0; i < nl; i++) { memcpy(L[i].pos, lights + 8 * i, 12); memcpy(L[i].color, lights + 8 * i + 3, 12); L[i].rad = lights[8 * i + 6]; L[i].shadow = lights[8 * i + 7] != 0; }
  HostStack hs;
  unsigned int err = 0;
  const bool exact = faithful || exact_traversal(s->rules.traits.has_refract, maxdepth);
  for (size_t i = 0; i < n; i++) {
    Ray r; r.o = v3(ox[i], oy[i], oz[i]); r.d = v3(dx[i], dy[i], dz[i]);
    if (tier == 0 && !exact && !unit_length(r.d)) return -4;  // (trace_batch_loop's CHECK: kErrNonUnit)
    float* o = out5 + 5 * i; unsigned int* c = counts2 + 2 * i;
    if (tier != 0) { HostGenericTier T{s->D, L, nl, Cnt()}; T.packets(); trace_one(T, r, tmax[i], maxdepth, o, c, err); }
    else if (exact && full) { HostFlatTier<true, false, true> T{s->D, L, nl, hs.lane(kFlatStack), Cnt()}; trace_one(T, r, tmax[i], maxdepth, o, c, err); }
    else if (exact) { HostFlatTier<true, false, false> T{s->D, L, nl, hs.lane(kFlatStack), Cnt()}; trace_one(T, r, tmax[i], maxdepth, o, c, err); }
    else if (full) { HostFlatTier<false, false, true> T{s->D, L, nl, hs.lane(kFlatStack), Cnt()}; trace_one(T, r, tmax[i], maxdepth, o, c, err); }
    else { HostFlatTier<false, false, false> T{s->D, L, nl, hs.lane(kFlatStack), Cnt()}; trace_one(T, r, tmax[i], maxdepth, o, c, err); }
  }
  return err ? -2 : 0;
}

// Diagnostic: per-lane traversal work inside each 8x8 pixel block (what one wave executes), for primary rays and for
// the shadow rays they spawn.  out[block][lane][k]: k = 0 nodes, 1 prim tests (primary); 2 nodes, 3 prims (shadow; -1 = no shadow ray)
int hostsim_block_work(void* sv, const float* cam, const float* light_pos, int width, int height, int* out) {
  SimScene* s = (SimScene*)sv;
  if (s->D.tier != 0) return -1;
  DCamera C; memcpy(&C, cam, sizeof(C));
  HostStack hs;
  int bw = width / 8, bh = height / 8;
  for (int by = 0; by < bh; by++) for (int bx = 0; bx < bw; bx++) for (int lane = 0; lane < 64; lane++) {
    int px = bx * 8 + (lane & 7), py = by * 8 + (lane >> 3);
    float xc, yc; get_coordsf(width, height, (float)px, (float)py, xc, yc);
    Ray ray = primary_ray(C, xc, yc);
    HostFlatTier<false, true, false> T{s->D, nullptr, 0, hs.lane(kFlatStack), Cnt()};
    HitG h = T.closest(ray, kInf);
    int* o = out + ((size_t)(by * bw + bx) * 64 + lane) * 4;
    o[0] = (int)T.cnt.bih; o[1] = (int)T.cnt.prim; o[2] = -1; o[3] = -1;
    if (h.hit) {
      V3 lvec = v3(light_pos[0], light_pos[1], light_pos[2]) - h.p;
      if (!(vdot(lvec, h.n) < 0)) {
        float llen = sqrtf(vdot(lvec, lvec));
        Ray sr; sr.o = vscaleadd(h.p, h.n, kDel); sr.d = lvec * (1.0f / llen);
        HostFlatTier<false, true, false> T2{s->D, nullptr, 0, hs.lane(kFlatStack), Cnt()};
        T2.occluded(sr, llen - 2 * kDel);
        o[2] = (int)T2.cnt.bih; o[3] = (int)T2.cnt.prim;
      }
    }
  }
  return 0;
}

// renderTileSubsample through the device headers' pass helpers (ss_candidate / ss_neighbours / ccmp / cavg / blend),
// executed sequentially tile by tile.  Mirrors ss_frame_loop in render_kernels.hpp.
int hostsim_render_subsample(void* sv, int tier, const float* cam, const float* lights, int nl, int width, int height, int maxdepth, int blocksize,
                             const float* thresholds, float* out5, unsigned long long* counters) {
  SimScene* s = (SimScene*)sv;
  if (tier < 0) tier = (int)s->D.tier;
  if (tier == 0 && s->D.tier != 0) return -1;
  DCamera C; memcpy(&C, cam, sizeof(C));
  DLight L[kMaxLights];
  for (int i = 0; i < nl; i++) { memcpy(L[i].pos, lights + 8 * i, 12); memcpy(L[i].color, lights + 8 * i + 3, 12); L[i].rad = lights[8 * i + 6]; L[i].shadow = lights[8 * i + 7] != 0; }
  HostStack hs;
  unsigned long long nprim = 0, nshadow = 0, nsec = 0;
  unsigned int err = 0;
  const bool exact = exact_traversal(refract_scene(s), maxdepth);
  auto sample = [&](float xp, float yp) {
    float xc, yc; get_coordsf(width, height, xp, yp, xc, yc);
    Ray ray = primary_ray(C, xc, yc);
    HitG h; CA c;
    nprim++;
    if (tier == 0 && exact) { HostFlatTier<true, false, true> T{s->D, L, nl, hs.lane(kFlatStack), Cnt()}; c = trace_primary(T, ray, kInf, maxdepth, true, &h); nshadow += T.cnt.shadow; nsec += T.cnt.secondary; }
    else if (tier == 0) { HostFlatTier<false, false, true> T{s->D, L, nl, hs.lane(kFlatStack), Cnt()}; c = trace_primary(T, ray, kInf, maxdepth, true, &h); nshadow += T.cnt.shadow; nsec += T.cnt.secondary; }
    else { HostGenericTier T{s->D, L, nl, Cnt()}; T.packets(); c = trace_primary(T, ray, kInf, maxdepth, true, &h); err |= T.err; nshadow += T.cnt.shadow; nsec += T.cnt.secondary; }
    return tc(c.r, c.g, c.b, c.a, h.hit ? h.t : kInf);
  };
  for (int xt = 0; xt < width;) {
    int tw = (xt + blocksize >= width) ? width - xt : blocksize;
    for (int yt = 0; yt < height;) {
      int th = (yt + blocksize >= height) ? height - yt : blocksize;
      std::vector<TC> v((size_t)tw * th, tc_blank());
      auto getc = [&](int dx, int dy) { return (dx >= 0 && dx < tw && dy >= 0 && dy < th) ? v[(size_t)dy * tw + dx] : tc_blank(); };
      for (int pass = 1; pass <= 5; pass++) {
        float thr = pass >= 2 ? thresholds[pass - 2] : 0.0f;
        int ox[4], oy[4];
        ss_neighbours(pass, ox, oy);
        std::vector<TC> nv = v;  // passes never read what they write, so a copy is equivalent and keeps this mirror simple
        for (int i = 0; i < tw * th; i++) {
          int dx = i % tw, dy = i / tw;
          if (!ss_candidate(pass, dx, dy)) continue;
          TC a = tc_blank(), b = a, c = a, d = a, col;
          bool need = true;
          if (pass >= 2) {
            a = getc(dx + ox[0], dy + oy[0]); b = getc(dx + ox[1], dy + oy[1]); c = getc(dx + ox[2], dy + oy[2]); d = getc(dx + ox[3], dy + oy[3]);
            need = gmaxf(ccmp(a, c), ccmp(b, d)) > thr;
          }
          float off = pass == 5 ? 0.5f : 0.0f;
          col = need ? sample((float)(xt + dx) + off, (float)(yt + dy) + off) : cavg4(a, b, c, d);
          if (pass < 5) nv[i] = col;
          else {
            TC o = ss_pass5_blend(col, a, b, c, d, dx == tw - 1, dy == th - 1);
            float* q = out5 + ((size_t)(yt + dy) * width + (xt + dx)) * 5;
            q[0] = o.r; q[1] = o.g; q[2] = o.b; q[3] = o.a; q[4] = o.d;
          }
        }
        v.swap(nv);
      }
      yt += th;
    }
    xt += tw;
  }
  if (counters) { counters[0] = nprim; counters[1] = nshadow; counters[2] = nsec; }
  return err ? -2 : 0;
}

// The adaptive sampler's item arithmetic, walked the way ss_frame_loop (render_kernels.hpp) walks it: ss_plan of a launch with
// this blocksize and these region shapes, then for every region r of a tile (rx = r % nrx, ry = r / nrx) its blocks inside a
// tw x th tile (ss_region_blocks), block b at (bx0 + b % nbx, by0 + b / nbx), and the candidate of each of its 64 lanes
// (ss_block_pixel).  pass: 1..5.  rw, rh: indexed by pass like DRenderArgs::ss_rw / ss_rh.
//   items (may be null): 5 ints per lane -- region, block, lane, dx, dy -- while they fit in cap_items entries
//   cover (may be null): 65 x 65 counts of how often a pixel with dx < tw and dy < th came up
//   plan  (may be null): per_tile[6], nrx[6], first[7], tiles_per_head, kSSHeads  (21 words)
// Returns the number of (region, block, lane) triples walked.  pass 0: all five passes, cover = 5 x 65 x 65 (no item list).
long long hostsim_ss_items(int pass, int blocksize, int tw, int th, const int* rw, const int* rh, int ntiles, int nframes,
                           int* items, long long cap_items, unsigned short* cover, unsigned int* plan) {
  if (pass == 0) {
    long long total = 0;
    for (int p = 1; p <= 5; p++) {
      const long long n = hostsim_ss_items(p, blocksize, tw, th, rw, rh, ntiles, nframes, nullptr, 0, cover ? cover + (p - 1) * 65 * 65 : nullptr, plan);
      if (n < 0) return n;
      total += n;
    }
    return total;
  }
  if (pass < 1 || pass > 5 || blocksize < 1 || blocksize > 65 || tw < 1 || th < 1 || tw > blocksize || th > blocksize) return -1;
  DRenderArgs A;
  memset(&A, 0, sizeof(A));
  A.blocksize = blocksize; A.ntiles = ntiles; A.nframes = nframes;
  for (int p = 1; p <= 5; p++) { A.ss_rw[p] = (int8_t)rw[p]; A.ss_rh[p] = (int8_t)rh[p]; }
  const SSPlan PL = ss_plan(A);
  if (plan) {
    for (int p = 0; p < 6; p++) { plan[p] = PL.per_tile[p]; plan[6 + p] = PL.nrx[p]; }
    for (int p = 0; p < 7; p++) plan[12 + p] = PL.first[p];
    plan[19] = PL.tiles_per_head; plan[20] = kSSHeads;
  }
  if (cover) memset(cover, 0, 65 * 65 * sizeof(unsigned short));
  long long n = 0;
  for (int r = 0; r < (int)PL.per_tile[pass]; r++) {
    const int rx = r % (int)PL.nrx[pass], ry = r / (int)PL.nrx[pass];
    int bx0, by0, nbx, nb;
    ss_region_blocks(pass, tw, th, rx, ry, A.ss_rw[pass], A.ss_rh[pass], bx0, by0, nbx, nb);
    for (int b = 0; b < nb; b++) {
      const int bx = bx0 + b % nbx, by = by0 + b / nbx;
      for (int lane = 0; lane < 64; lane++, n++) {
        int dx, dy;
        ss_block_pixel(pass, bx, by, lane, dx, dy);
        if (items && n < cap_items) { int* o = items + 5 * n; o[0] = r; o[1] = b; o[2] = lane; o[3] = dx; o[4] = dy; }
        if (cover && dx < tw && dy < th) {
          if (dx < 0 || dy < 0) return -2;
          cover[dy * 65 + dx]++;
        }
      }
    }
  }
  return n;
}
// ss_region_shape (rt_device.hpp): the flat tier's region of pass p at size 0, 1, 2
void hostsim_ss_region_shape(int pass, int size, int* rw, int* rh) { int a, b; ss_region_shape(pass, size, a, b); *rw = a; *rh = b; }
}
