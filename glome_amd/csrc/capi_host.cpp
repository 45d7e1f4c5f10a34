// capi_host.cpp -- host half of the C ABI (include/glome_hip.h): the scene builder (one call per glome
// constructor), the transform helpers and the host-side inspection calls (among them the choice of a kernel instance, instances.hpp).
// No HIP here.
#include <algorithm>
#include <array>
#include <cstdlib>
#include <cstring>
#include <string>

#include "../../include/glome_hip.h"
#include "capi_shared.hpp"
#include "show_format.hpp"
#include "tiles.hpp"
#include "xfm_sources.hpp"

using namespace glome;

namespace {
D3 d3(const double* p) { return D3{p[0], p[1], p[2]}; }
Xf xf_from(const double* m) { Xf x; for (int k = 0; k < 12; k++) { x.f.m[k] = m[k]; x.i.m[k] = m[12 + k]; } return x; }
void xf_to(const Xf& x, double* out) { for (int k = 0; k < 12; k++) { out[k] = x.f.m[k]; out[12 + k] = x.i.m[k]; } }

template <class F> int32_t guard(glome_sb* sb, F f) {
  if (!sb) return GLOME_E_INVALID;
  try { return (int32_t)f(); }
  catch (const scene_error& e) { sb->err = e.what(); return GLOME_E_SCENE; }
  catch (const limit_error& e) { sb->err = e.what(); return GLOME_E_LIMIT; }
  catch (const std::invalid_argument& e) { sb->err = e.what(); return GLOME_E_INVALID; }
  catch (const std::exception& e) { sb->err = e.what(); return GLOME_E_INVALID; }
}
template <class F> int xguard(F f) {
  try { f(); return 0; } catch (...) { return GLOME_E_SCENE; }
}
std::vector<int> ids_of(const int32_t* ids, int n) {
  if (n < 0 || (n > 0 && !ids)) throw std::invalid_argument("bad id list");
  return std::vector<int>(ids, ids + n);
}
}  // namespace

extern "C" {

void glome_render_params_default(glome_render_params* p) {
  if (!p) return;
  memset(p, 0, sizeof(*p));
  p->width = 720; p->height = 480;         // Glome.hs:112-113
  p->mode = GLOME_MODE_TILE;
  p->blocksize = 65;                       // Glome.hs:116
  p->maxdepth = 3;                         // Glome.hs:25
  p->thresholds[0] = 0.14f; p->thresholds[1] = 0.15f; p->thresholds[2] = 0.16f; p->thresholds[3] = 0.18f;  // Glome.hs:221-224
  p->tile_first = 0; p->tile_stride = 1; p->rank0_share_pct = 0;
}

void glome_trace_params_default(glome_trace_params* p) {
  if (!p) return;
  memset(p, 0, sizeof(*p));
  p->maxdepth = 3;  // Glome.hs:25
}

// ---- the lens stages' host-only entries (the rest: runtime.hip) ----
static_assert((int)GLOME_LENS_PINHOLE == (int)LENS_PINHOLE && (int)GLOME_LENS_THIN == (int)LENS_THIN && (int)GLOME_LENS_LATLONG == (int)LENS_LATLONG, "the header's lenses are the kernels' (rt_types.h)");
void glome_raygen_params_default(glome_raygen_params* p) {
  if (!p) return;
  memset(p, 0, sizeof(*p));
  p->width = 720; p->height = 480;  // Glome.hs:112-113
  p->lens = GLOME_LENS_PINHOLE;
  p->samples = 1;
  p->focus_dist = 1.0f;
}
size_t glome_raygen_params_size(void) { return sizeof(glome_raygen_params); }
int64_t glome_raygen_count(const glome_raygen_params* p) {
  if (raygen_params_error(p)) return GLOME_E_INVALID;
  return (int64_t)p->width * p->height * p->samples;
}
uint32_t glome_raygen_sample(uint32_t seed, uint32_t pixel, uint32_t s, uint32_t dim) { return raygen_word(seed, pixel, s, dim); }

// ---- the adaptive rule's host-only entries (adaptive_rule.hpp: the bodies the fold kernels compile; the device path: runtime.hip) ----
void glome_adaptive_params_default(glome_adaptive_params* p) {
  if (!p) return;
  memset(p, 0, sizeof(*p));
  p->base_samples = 4; p->threshold = 1.0f / 64;  // a first guess, not tuned
}
size_t glome_adaptive_params_size(void) { return sizeof(glome_adaptive_params); }
int glome_adaptive_levels(int32_t base, int32_t max, int32_t* out, int cap) {
  if (!adaptive::legal(base, max) || cap < 0 || (cap > 0 && !out)) return GLOME_E_INVALID;
  int k = 0;
  for (int32_t n = base; n <= max; n *= 2, k++) if (k < cap) out[k] = n;
  return k;
}
namespace {
// rgbf (rt_device.hpp, Glome.hs:98-110) on the host: the float-to-int conversion spelled as the device's instruction performs it
// (saturating, 0 for a NaN), the word wrapping like Word32 arithmetic
uint32_t rgbf_channel(float x) {
  x = x >= 1 ? 1 - 0.0001f : x;  // cap1, kDel
  const float v = std::floor(x * 256);
  if (v != v) return 0u;
  if (v >= 2147483648.0f) return 0x7fffffffu;
  if (v <= -2147483648.0f) return 0x80000000u;
  return (uint32_t)(int32_t)v;
}
uint32_t rgbf_host(float r, float g, float b) { return rgbf_channel(r) * 65536u + rgbf_channel(g) * 256u + rgbf_channel(b); }
}  // namespace
int glome_adaptive_fold(const float* tuples, int32_t base, int32_t max, float threshold, int32_t* count, float rgbad[5], uint32_t* packed) {
  if (!tuples || !count || !rgbad || !packed || adaptive_rule_error(base, max, threshold)) return GLOME_E_INVALID;
  adaptive::Fold F = {};
  int32_t s = 0, n = base;
  for (;; n *= 2) {
    const uint32_t h = (uint32_t)n / 2;
    for (; s < n; s++) adaptive::take(F, (uint32_t)s, h, tuples + 5 * (size_t)s);
    if (n == max || adaptive::agrees(F, h, threshold)) break;
  }
  adaptive::result(F, (uint32_t)n, rgbad);
  *count = n;
  *packed = rgbf_host(rgbad[0] * rgbad[3], rgbad[1] * rgbad[3], rgbad[2] * rgbad[3]);
  return 0;
}

int glome_xfm_translate(const double v[3], double out[24]) { return xguard([&] { xf_to(xf_translate(d3(v)), out); }); }
int glome_xfm_scale(const double v[3], double out[24]) { return xguard([&] { xf_to(xf_scale(d3(v)), out); }); }
int glome_xfm_rotate(const double axis[3], double angle, double out[24]) { return xguard([&] { xf_to(xf_rotate(d3(axis), angle), out); }); }
int glome_xfm_xyz_to_uvw(const double u[3], const double v[3], const double w[3], double out[24]) { return xguard([&] { xf_to(xf_xyz_to_uvw(d3(u), d3(v), d3(w)), out); }); }
int glome_xfm_compose(const double* xfms, int n, double out[24]) {
  return xguard([&] { std::vector<Xf> xs; for (int k = 0; k < n; k++) xs.push_back(xf_from(xfms + 24 * k)); xf_to(xf_compose(xs), out); });
}
// The matrices of glome_scene_instance_update_from's forms (xfm_sources.hpp: the conversion kernel's own bodies).
int glome_xfm_from_forward(const double m12[12], double out[24]) {
  if (!m12 || !out) return GLOME_E_INVALID;
  for (int q = 0; q < 12; q++) if (!std::isfinite(m12[q])) return GLOME_E_INVALID;
  double o[24];
  const double det = xfm::from_forward(m12, o);
  bool finite = true;
  for (int q = 12; q < 24; q++) finite = finite && std::isfinite(o[q]);
  if (det == 0.0 || !finite) return GLOME_E_SCENE;
  std::copy(o, o + 24, out);
  return 0;
}
int glome_xfm_from_pose(const double t[3], const double q_xyzw[4], double s, double out[24]) {
  if (!t || !q_xyzw || !out) return GLOME_E_INVALID;
  const double p[8] = {t[0], t[1], t[2], q_xyzw[0], q_xyzw[1], q_xyzw[2], q_xyzw[3], s};
  for (int q = 0; q < 8; q++) if (!std::isfinite(p[q])) return GLOME_E_INVALID;
  double o[24];
  if (!xfm::from_pose(p, o)) return GLOME_E_INVALID;
  for (int q = 0; q < 24; q++) if (!std::isfinite(o[q])) return GLOME_E_INVALID;
  std::copy(o, o + 24, out);
  return 0;
}
int glome_xfm_mult(const double a[24], const double b[24], double out[24]) {
  if (!a || !b || !out) return GLOME_E_INVALID;
  double o[24];
  xfm::mult(a, b, o);
  std::copy(o, o + 24, out);
  return 0;
}
int glome_camera_lookat(const double pos[3], const double at[3], const double up[3], double angle_deg, glome_camera* out) {  // Scene.hs:48-57
  if (!out) return GLOME_E_INVALID;
  D3 p = d3(pos);
  D3 fwd = normalize(d3(at) - p);
  D3 right = normalize(cross(d3(up), fwd));
  D3 up_ = normalize(cross(fwd, right));
  double cam_scale = std::tan((M_PI / 180) * (angle_deg / 2));
  D3 u = up_ * cam_scale, r = right * cam_scale;
  const D3 v[4] = {p, fwd, u, r};
  float* o = out->pos;
  for (int k = 0; k < 4; k++) { o[3 * k] = (float)v[k].x; o[3 * k + 1] = (float)v[k].y; o[3 * k + 2] = (float)v[k].z; }
  return 0;
}

int glome_tex_words(void) { return GLOME_TEX_WORDS; }  // int32 words per ray of glome_rayint_batch's texture-stack output
static_assert(GLOME_WORK_WORDS == kWorkWords && GLOME_WORK_PRIMARY_PRIM_TESTS == kWorkWords - 1, "the header's work record is the kernels' (rt_types.h, trace_kernels.hpp)");
int glome_work_words(void) { return GLOME_WORK_WORDS; }  // uint32 words per ray of glome_trace_work_batch's records

glome_sb* glome_sb_new(void) { return new glome_sb(); }
void glome_sb_free(glome_sb* sb) { delete sb; }
const char* glome_sb_last_error(const glome_sb* sb) { return sb ? sb->err.c_str() : "null builder"; }

int32_t glome_sb_sphere(glome_sb* sb, const double c[3], double r) { return guard(sb, [&] { return sb->graph.sphere(d3(c), r); }); }
int32_t glome_sb_triangle(glome_sb* sb, const double p[9]) { return guard(sb, [&] { return sb->graph.triangle(d3(p), d3(p + 3), d3(p + 6)); }); }
int32_t glome_sb_trianglenorm(glome_sb* sb, const double p[9], const double n[9]) {
  return guard(sb, [&] { return sb->graph.trianglenorm(d3(p), d3(p + 3), d3(p + 6), d3(n), d3(n + 3), d3(n + 6)); });
}
int32_t glome_sb_box(glome_sb* sb, const double a[3], const double b[3]) { return guard(sb, [&] { return sb->graph.box(d3(a), d3(b)); }); }
int32_t glome_sb_plane(glome_sb* sb, const double pt[3], const double n[3]) { return guard(sb, [&] { return sb->graph.plane(d3(pt), d3(n)); }); }
int32_t glome_sb_plane_offset(glome_sb* sb, const double n[3], double off) { return guard(sb, [&] { return sb->graph.plane_offset(d3(n), off); }); }
int32_t glome_sb_disc(glome_sb* sb, const double pos[3], const double n[3], double r) { return guard(sb, [&] { return sb->graph.disc(d3(pos), d3(n), r); }); }
int32_t glome_sb_cylinder(glome_sb* sb, const double p1[3], const double p2[3], double r) { return guard(sb, [&] { return sb->graph.cylinder(d3(p1), d3(p2), r); }); }
int32_t glome_sb_cone(glome_sb* sb, const double p1[3], double r1, const double p2[3], double r2) { return guard(sb, [&] { return sb->graph.cone(d3(p1), r1, d3(p2), r2); }); }
int32_t glome_sb_group(glome_sb* sb, const int32_t* ids, int n) { return guard(sb, [&] { return sb->graph.group(ids_of(ids, n)); }); }
int32_t glome_sb_transform(glome_sb* sb, int32_t id, const double* xfms, int n) {
  return guard(sb, [&] {
    if (n < 0 || (n > 0 && !xfms)) throw std::invalid_argument("bad transform list");
    std::vector<Xf> xs;
    for (int k = 0; k < n; k++) xs.push_back(xf_from(xfms + 24 * k));
    return sb->graph.transform(id, xs);
  });
}
int32_t glome_sb_difference(glome_sb* sb, int32_t a, int32_t b) { return guard(sb, [&] { return sb->graph.difference(a, b); }); }
int32_t glome_sb_difference_retexture(glome_sb* sb, int32_t a, int32_t b) { return guard(sb, [&] { return sb->graph.difference(a, b, true); }); }
int32_t glome_sb_intersection(glome_sb* sb, const int32_t* ids, int n) { return guard(sb, [&] { return sb->graph.intersection(ids_of(ids, n)); }); }
int32_t glome_sb_bih(glome_sb* sb, const int32_t* ids, int n) { return guard(sb, [&] { return sb->graph.bih(ids_of(ids, n)); }); }
int glome_sb_bih_set_triangles(glome_sb* sb, int32_t bih_id, const double* pts9, int n) {
  return guard(sb, [&] {
    if (n < 0 || (n && !pts9)) throw std::invalid_argument("bih_set_triangles: null triangle array");
    std::vector<D3> P;
    for (size_t k = 0; k < 3 * (size_t)n; k++) P.push_back(d3(pts9 + 3 * k));
    sb->graph.bih_set_triangles(bih_id, P);
    return 0;
  });
}
int glome_sb_bih_set_triangles_indexed(glome_sb* sb, int32_t bih_id, const double* verts, int nv, const int32_t* idx3, int n) {
  return guard(sb, [&] {
    if (n < 0 || nv < 0 || (n && !idx3) || (nv && !verts)) throw std::invalid_argument("bih_set_triangles_indexed: null vertex or index array");
    std::vector<D3> P;  // the gathered array: only referenced vertices are looked at
    for (size_t k = 0; k < 3 * (size_t)n; k++) {
      const int32_t i = idx3[k];
      if (i < 0 || i >= nv) throw std::invalid_argument("bih_set_triangles_indexed: item " + std::to_string(k / 3) + " has vertex index " + std::to_string(i) + ", outside [0, " + std::to_string(nv) + ")");
      P.push_back(d3(verts + 3 * (size_t)i));
    }
    sb->graph.bih_set_triangles(bih_id, P);
    return 0;
  });
}
int glome_sb_bih_set_spheres(glome_sb* sb, int32_t bih_id, const double* c3r, int n) {
  return guard(sb, [&] {
    if (n < 0 || (n && !c3r)) throw std::invalid_argument("bih_set_spheres: null sphere array");
    sb->graph.bih_set_spheres(bih_id, std::vector<double>(c3r, c3r + 4 * (size_t)n));
    return 0;
  });
}
int glome_sb_instance_set_transforms(glome_sb* sb, const int32_t* ids, const double* xfms, int n) {
  return guard(sb, [&] {
    if (n < 0 || (n && (!ids || !xfms))) throw std::invalid_argument("instance_set_transforms: bad count or null array");
    std::vector<Xf> X;
    for (int k = 0; k < n; k++) X.push_back(xf_from(xfms + 24 * (size_t)k));
    sb->graph.instance_set_transforms(std::vector<int>(ids, ids + n), X);
    return 0;
  });
}
int glome_sb_instance_transform(glome_sb* sb, int32_t id, double out[24]) {
  return guard(sb, [&] {
    if (!out) throw std::invalid_argument("instance_transform: null output");
    const Node& n = sb->graph.at(id);
    if (n.kind != K_INSTANCE) throw std::invalid_argument("instance_transform: node " + std::to_string(id) + " is a " + kind_name(n.kind) + ", not an Instance");
    xf_to(n.xf, out);
    return 0;
  });
}
int glome_sb_bih_refit(glome_sb* sb, int32_t bih_id) {
  return guard(sb, [&] {
    Graph& G = sb->graph;
    if (G.at(bih_id).kind != K_BIH) throw std::invalid_argument(std::string("bih_refit: node ") + std::to_string(bih_id) + " is a " + kind_name(G.at(bih_id).kind) + ", not a Bih");
    Box3 bb = box_empty();  // the constructor's own refusal (`bih`), before the tree is touched
    for (int it : G.at(bih_id).bih->update_order()) bb = box_join(bb, G.bound(it));
    if (bb.lo.x == -kInfinity || bb.lo.y == -kInfinity || bb.lo.z == -kInfinity || bb.hi.x == kInfinity || bb.hi.y == kInfinity || bb.hi.z == kInfinity)
      throw scene_error("bih_refit: bih " + std::to_string(bih_id) + ": bih: infinite bounding box");
    G.bih_refit(bih_id);
    return 0;
  });
}
int glome_sb_bih_resplit(glome_sb* sb, int32_t bih_id) {
  return guard(sb, [&] {
    sb->graph.bih_resplit(bih_id);
    return 0;
  });
}
int glome_sb_bih_layout(glome_sb* sb, int32_t bih_id, int64_t out4[4]) {
  return guard(sb, [&] {
    if (!out4) throw std::invalid_argument("bih_layout: null output");
    const Graph& G = sb_graph(sb);
    if (G.at(bih_id).kind != K_BIH) throw std::invalid_argument(std::string("bih_layout: node ") + std::to_string(bih_id) + " is a " + kind_name(G.at(bih_id).kind) + ", not a Bih");
    FlatScene F;  // the commit's own layout, of a scene that is only this tree
    Flattener fl(G, F);
    fl.run(bih_id);
    for (const LeafBihUpdateInfo& U : F.leaf_bih_updates) {
      if (U.node != bih_id) continue;
      out4[0] = U.n_slots; out4[1] = U.n_pair_recs; out4[2] = U.n_recs; out4[3] = U.depth;
      return 0;
    }
    throw std::invalid_argument("bih_layout: bih " + std::to_string(bih_id) + " is not a leaf bih: its items are not all plain triangles or all plain spheres");
  });
}
int32_t glome_sb_bihs_above(glome_sb* sb, int32_t root, int32_t node_id, int32_t* out, int32_t cap) {
  return guard(sb, [&] {
    FlatScene F;
    Flattener fl(sb_graph(sb), F);
    fl.run(root);
    const NestedAnswer* A = nullptr;
    for (const MeshUpdateInfo& U : F.mesh_updates) if (U.node == node_id) A = &U.nested;
    for (const LeafBihUpdateInfo& U : F.leaf_bih_updates) if (U.node == node_id) A = &U.nested;
    for (const InstanceUpdateInfo& U : F.inst_updates) if (U.node == node_id) A = &U.nested;
    for (const InstBihInfo& B : F.inst_bihs) if (B.node == node_id) A = &B.nested;
    if (!A) throw std::invalid_argument("bihs_above: node " + std::to_string(node_id) + " is not a Mesh, a triangle bih, an Instance or a refittable bih of the scene under node " + std::to_string(root) + " (nor a sphere bih)");
    if (!A->ok) throw std::invalid_argument("bihs_above: " + A->why_not);
    for (size_t k = 0; k < A->above.size() && (int32_t)k < cap && out; k++) out[k] = A->above[k];
    return (int)A->above.size();
  });
}
int32_t glome_sb_bih_items(glome_sb* sb, int32_t bih_id, int32_t* out, int32_t cap) {
  return guard(sb, [&] {
    const Node& n = sb->graph.at(bih_id);
    if (n.kind != K_BIH) throw std::invalid_argument(std::string("bih_items: node ") + std::to_string(bih_id) + " is a " + kind_name(n.kind) + ", not a Bih");
    const std::vector<int> items = n.bih->update_order();
    for (size_t k = 0; k < items.size() && (int32_t)k < cap && out; k++) out[k] = items[k];
    return (int)items.size();
  });
}
int32_t glome_sb_mesh(glome_sb* sb, const double* verts, int nv, const double* norms, int nn, const int32_t* tris, int nt, const int32_t* mats, int nm) {
  return guard(sb, [&] {
    if (nv < 0 || nn < 0 || nt < 0 || nm < 0 || (nv && !verts) || (nn && !norms) || (nt && !tris) || (nm && !mats)) throw std::invalid_argument("bad mesh arrays");
    std::vector<D3> V, N;
    for (int k = 0; k < nv; k++) V.push_back(d3(verts + 3 * k));
    for (int k = 0; k < nn; k++) N.push_back(d3(norms + 3 * k));
    std::vector<MeshTri> T;
    for (int k = 0; k < nt; k++) { const int32_t* t = tris + 8 * k; T.push_back(MeshTri{t[0], t[1], t[2], t[3], t[4], t[5], t[6], t[7]}); }
    return sb->graph.mesh(std::move(V), std::move(N), std::move(T), std::vector<int>(mats, mats + nm));
  });
}
int glome_sb_mesh_set_vertices(glome_sb* sb, int32_t mesh_id, const double* verts, int nv, const double* norms, int nn) {
  return guard(sb, [&] {
    if (nv < 0 || nn < 0 || (nv && !verts) || (nn && !norms)) throw std::invalid_argument("mesh_set_vertices: bad vertex / normal arrays");
    std::vector<D3> V, N;
    for (int k = 0; k < nv; k++) V.push_back(d3(verts + 3 * k));
    for (int k = 0; k < nn; k++) N.push_back(d3(norms + 3 * k));
    sb->graph.mesh_set_vertices(mesh_id, std::move(V), std::move(N));
    return 0;
  });
}
int32_t glome_sb_tex(glome_sb* sb, int32_t id, int32_t material) { return guard(sb, [&] { return sb->graph.wrap(K_TEX, id, material); }); }
int32_t glome_sb_tag(glome_sb* sb, int32_t id) { return guard(sb, [&] { return sb->graph.wrap(K_TAG, id); }); }
int32_t glome_sb_noshadow(glome_sb* sb, int32_t id) { return guard(sb, [&] { return sb->graph.wrap(K_NOSHADOW, id); }); }
int32_t glome_sb_onlyshadow(glome_sb* sb, int32_t id) { return guard(sb, [&] { return sb->graph.wrap(K_ONLYSHADOW, id); }); }
int32_t glome_sb_bound_object(glome_sb* sb, int32_t a, int32_t b) { return guard(sb, [&] { return sb->graph.bound_object(a, b, false); }); }
int32_t glome_sb_innerbound(glome_sb* sb, int32_t a, int32_t b) { return guard(sb, [&] { return sb->graph.bound_object(a, b, true); }); }
int32_t glome_sb_flatten_transform(glome_sb* sb, int32_t id) { return guard(sb, [&] { return sb->graph.flatten_transform_item(id); }); }
int32_t glome_sb_tolist(glome_sb* sb, int32_t id) { return guard(sb, [&] { return sb->graph.tolist_node(id); }); }
int32_t glome_sb_list_items(glome_sb* sb, int32_t id, int32_t* out, int32_t cap) {
  return guard(sb, [&] {
    std::vector<int> items;
    sb->graph.tolist(id, items);
    for (size_t k = 0; k < items.size() && (int32_t)k < cap && out; k++) out[k] = items[k];
    return (int)items.size();
  });
}

int32_t glome_sb_material_surface(glome_sb* sb, const double color[3], double alpha, double amb, double kd, double ks, double shine) {
  return guard(sb, [&] { Mat m; m.kind = MAT_SURFACE; m.color[0] = color[0]; m.color[1] = color[1]; m.color[2] = color[2]; m.alpha = alpha; m.amb = amb; m.kd = kd; m.ks = ks; m.shine = shine; return sb->graph.add_mat(m); });
}
int32_t glome_sb_material_reflect(glome_sb* sb, double refl) { return guard(sb, [&] { Mat m; m.kind = MAT_REFLECT; m.refl = refl; return sb->graph.add_mat(m); }); }
int32_t glome_sb_material_refract(glome_sb* sb, double refl, double refr, double ior) {
  return guard(sb, [&] { Mat m; m.kind = MAT_REFRACT; m.refl = refl; m.refr = refr; m.ior = ior; return sb->graph.add_mat(m); });
}
int32_t glome_sb_material_layers(glome_sb* sb, const int32_t* mats, int n) {
  return guard(sb, [&] { Mat m; m.kind = MAT_LAYERS; m.kids = ids_of(mats, n); for (int k : m.kids) sb->graph.check_mat(k); return sb->graph.add_mat(m); });
}
int32_t glome_sb_material_blend(glome_sb* sb, int32_t a, int32_t b, double weight) {
  return guard(sb, [&] { sb->graph.check_mat(a); sb->graph.check_mat(b); Mat m; m.kind = MAT_BLEND; m.a = a; m.b = b; m.weight = weight; return sb->graph.add_mat(m); });
}
int32_t glome_sb_material_blend_fn(glome_sb* sb, int32_t a, int32_t b, int32_t weight_fn, const double* params4) {
  return guard(sb, [&] {
    sb->graph.check_mat(a); sb->graph.check_mat(b);
    if (weight_fn < GLOME_WEIGHT_PERLIN || weight_fn > GLOME_WEIGHT_STRIPE_SINE || !params4) throw std::invalid_argument("bad weight function");
    Mat m; m.kind = MAT_BLEND; m.a = a; m.b = b; m.wfn = weight_fn;
    for (int k = 0; k < 4; k++) m.wp[k] = params4[k];
    return sb->graph.add_mat(m);
  });
}

int32_t glome_sb_material_warp(glome_sb* sb, int32_t frame, int32_t scene, const glome_light* lights, int nlights, const double xfm[24]) {
  return guard(sb, [&] {
    if (nlights < 0 || nlights > kMaxLights || (nlights > 0 && !lights) || !xfm) throw std::invalid_argument("bad Warp lights / transform");
    sb->graph.at(frame);
    if (scene >= 0) sb->graph.at(scene);
    Mat m; m.kind = MAT_WARP; m.wframe = frame; m.wscene = scene < 0 ? -1 : scene; m.wxf = xf_from(xfm);
    for (int k = 0; k < nlights; k++) {
      WarpLight L;
      for (int q = 0; q < 3; q++) { L.pos[q] = lights[k].pos[q]; L.color[q] = lights[k].color[q]; }
      L.rad = lights[k].rad; L.shadow = lights[k].shadow != 0;
      m.wlights.push_back(L);
    }
    return sb->graph.add_mat(m);
  });
}

int glome_sb_primcount(glome_sb* sb, int32_t id, long out3[3]) {
  return guard(sb, [&] { out3[0] = out3[1] = out3[2] = 0; sb->graph.primcount(id, out3); return 0; });
}
int glome_sb_bound(glome_sb* sb, int32_t id, double out6[6]) {
  return guard(sb, [&] { Box3 b = sb->graph.bound(id); out6[0] = b.lo.x; out6[1] = b.lo.y; out6[2] = b.lo.z; out6[3] = b.hi.x; out6[4] = b.hi.y; out6[5] = b.hi.z; return 0; });
}
// ---- NFF / SPD scenes (GlomeTrace/Data/Glome/Spd.hs:89-254) ----
// A restatement of the reference's Read instances: whitespace-separated tokens, `#` starts a comment that runs to the
// end of the line (lexcr / lexignore, Spd.hs:13-30); statements v / l / b / f / s / c / p / pp; everything else ends
// the parse like accum_rss's fall-through (Spd.hs:212-242).
namespace {
struct NffLex {
  const char* p;
  explicit NffLex(const char* t) : p(t) {}
  void skip() {
    for (;;) {
      while (*p == ' ' || *p == '\t' || *p == '\r' || *p == '\n') p++;
      if (*p == '#') { while (*p && *p != '\n') p++; continue; }
      return;
    }
  }
  bool word(std::string& w) {  // the next token, not consumed unless accepted by the caller
    skip();
    const char* q = p;
    while (*q && !(*q == ' ' || *q == '\t' || *q == '\r' || *q == '\n')) q++;
    w.assign(p, q);
    return !w.empty();
  }
  void take(const std::string& w) { p += w.size(); }
  bool number(double& v) {  // reads :: Flt -- a token that parses completely as a number
    std::string w;
    if (!word(w)) return false;
    char* end = nullptr;
    double x = std::strtod(w.c_str(), &end);
    if (end == w.c_str() || *end != 0) return false;
    if (!((w[0] >= '0' && w[0] <= '9') || ((w[0] == '-') && w.size() > 1 && w[1] >= '0' && w[1] <= '9'))) return false;  // Haskell wants a leading digit
    take(w); v = x;
    return true;
  }
  bool vec(D3& v) { const char* save = p; if (number(v.x) && number(v.y) && number(v.z)) return true; p = save; return false; }
  bool keyword(const char* k) { std::string w; if (word(w) && w == k) { take(w); return true; } return false; }
};
}  // namespace

// `show geom` text (show_format.hpp)
long glome_sb_show(glome_sb* sb, int32_t id, char* buf, long cap) {
  if (!sb) return GLOME_E_INVALID;
  try {
    std::string o;
    ShowWriter W{sb->graph, o};
    W.item(id);
    if (buf && cap > 0) { size_t n = std::min<size_t>(o.size(), (size_t)cap - 1); memcpy(buf, o.data(), n); buf[n] = 0; }
    return (long)o.size();
  } catch (const std::exception& e) { sb->err = e.what(); return GLOME_E_INVALID; }
}
long glome_sb_show_tex_materials(glome_sb* sb, int32_t id, int32_t* mats, long cap) {
  if (!sb) return GLOME_E_INVALID;
  try {
    std::string o;
    std::vector<int> m;
    ShowWriter W{sb->graph, o, &m};
    W.item(id);
    for (long k = 0; mats && k < cap && k < (long)m.size(); k++) mats[k] = m[(size_t)k];
    return (long)m.size();
  } catch (const std::exception& e) { sb->err = e.what(); return GLOME_E_INVALID; }
}
int32_t glome_sb_load_show(glome_sb* sb, const char* text, const int32_t* tex_materials, int32_t n_tex_materials, int32_t default_material, int32_t* n_tex) {
  return guard(sb, [&] {
    if (!text) throw std::invalid_argument("null show text");
    if (n_tex_materials < 0 || (n_tex_materials > 0 && !tex_materials)) throw std::invalid_argument("bad material list");
    std::vector<int> mats(tex_materials, tex_materials + n_tex_materials);
    int nt = 0;
    int root = load_show(sb->graph, text, strlen(text), mats.data(), (int)mats.size(), default_material, &nt);
    if (n_tex) *n_tex = nt;
    return root;
  });
}

int32_t glome_sb_load_nff(glome_sb* sb, const char* text, double cam_from_at_up_angle[10], double* light_pos_rgb, int32_t max_lights, int32_t* n_lights,
                          double bg_rgb[3]) {
  return guard(sb, [&] {
    if (!text) throw std::invalid_argument("null NFF text");
    Graph& G = sb->graph;
    NffLex L(text);
    std::vector<int> groups;               // `tex (bih prims) fill`, in order of appearance
    std::vector<std::array<double, 6>> lights;
    bool have_cam = false, have_bg = false;
    double cam[10] = {0}, bg[3] = {0, 0, 0};
    int fill = -1;
    std::vector<int> prims;
    auto close_group = [&] { if (fill >= 0) groups.push_back(G.wrap(K_TEX, G.bih(prims), fill)); prims.clear(); };
    for (;;) {
      std::string w;
      if (!L.word(w)) break;
      const char* save = L.p;
      if (w == "v") {  // Spd.hs:89-107
        L.take(w);
        D3 from, at, up; double angle, skipn;
        std::string tok;
        bool ok = L.keyword("from") && L.vec(from) && L.keyword("at") && L.vec(at) && L.keyword("up") && L.vec(up) && L.keyword("angle") && L.number(angle) &&
                  L.keyword("hither") && L.word(tok);
        if (ok) { L.take(tok); ok = L.keyword("resolution") && L.word(tok); }
        if (ok) { L.take(tok); ok = L.word(tok); }
        if (ok) L.take(tok);
        (void)skipn;
        if (!ok) { L.p = save; break; }
        double c[10] = {from.x, from.y, from.z, at.x, at.y, at.z, up.x, up.y, up.z, angle};
        memcpy(cam, c, sizeof(c)); have_cam = true;  // the last camera of the file wins (accum_rss conses)
      } else if (w == "l") {  // Spd.hs:131-139: colour optional, default white
        L.take(w);
        D3 pos, c{1, 1, 1};
        if (!L.vec(pos)) { L.p = save; break; }
        D3 cc; if (L.vec(cc)) c = cc;
        lights.push_back({pos.x, pos.y, pos.z, c.x, c.y, c.z});
      } else if (w == "b") {  // Spd.hs:123-128
        L.take(w);
        D3 c; if (!L.vec(c)) { L.p = save; break; }
        bg[0] = c.x; bg[1] = c.y; bg[2] = c.z; have_bg = true;
      } else if (w == "f") {  // Spd.hs:141-153: Surface clr (1 - T) 0 kd ks shine
        L.take(w);
        D3 c; double kd, ks, shine, trans, ior;
        if (!(L.vec(c) && L.number(kd) && L.number(ks) && L.number(shine) && L.number(trans) && L.number(ior))) { L.p = save; break; }
        close_group();
        Mat m; m.kind = MAT_SURFACE; m.color[0] = c.x; m.color[1] = c.y; m.color[2] = c.z; m.alpha = 1 - trans; m.amb = 0; m.kd = kd; m.ks = ks; m.shine = shine;
        fill = G.add_mat(m);
      } else if (w == "s" || w == "c" || w == "p" || w == "pp") {  // Spd.hs:165-182
        if (fill < 0) break;  // a primitive needs a fill before it (readsSpdTextureGroup reads the texture first)
        L.take(w);
        if (w == "s") { D3 c; double r; if (!(L.vec(c) && L.number(r))) { L.p = save; break; } prims.push_back(G.sphere(c, r)); }
        else if (w == "c") { D3 a, b; double ra, rb; if (!(L.vec(a) && L.number(ra) && L.vec(b) && L.number(rb))) { L.p = save; break; } prims.push_back(G.cone(a, ra, b, rb)); }
        else {
          double n;
          if (!L.number(n)) { L.p = save; break; }  // the count is read and ignored: vertices are taken while they parse
          std::vector<D3> vs, ns;
          for (;;) {
            D3 v, nn;
            if (!L.vec(v)) break;
            if (w == "pp") { if (!L.vec(nn)) break; ns.push_back(nn); }
            vs.push_back(v);
          }
          std::vector<int> fan;  // triangles / trianglesnorms: a fan around the first vertex (Triangle.hs:28-42)
          for (size_t k = 1; k + 1 < vs.size(); k++)
            fan.push_back(w == "p" ? G.triangle(vs[0], vs[k], vs[k + 1]) : G.trianglenorm(vs[0], vs[k], vs[k + 1], ns[0], ns[k], ns[k + 1]));
          prims.push_back(G.group(fan));
        }
      } else break;
    }
    close_group();
    if (!have_cam) throw scene_error("NFF: no camera (v) statement");  // readsSpdScene's pattern needs one (Spd.hs:251)
    if (!have_bg) throw scene_error("NFF: no background (b) statement");
    std::reverse(groups.begin(), groups.end());  // accum_rss conses: the scene's list is in reverse order of appearance
    std::reverse(lights.begin(), lights.end());
    if (cam_from_at_up_angle) memcpy(cam_from_at_up_angle, cam, sizeof(cam));
    if (bg_rgb) memcpy(bg_rgb, bg, sizeof(bg));
    if (n_lights) *n_lights = (int32_t)lights.size();
    for (int k = 0; k < (int)lights.size() && k < max_lights && light_pos_rgb; k++) memcpy(light_pos_rgb + 6 * k, lights[k].data(), 6 * sizeof(double));
    return G.bih(groups);  // SPD (bih prims) lights cam bgc, Spd.hs:252
  });
}

long glome_sb_bih_dump(glome_sb* sb, int32_t id, long cap, double* lsplit, double* rsplit, int* axis, int* nleaf, int32_t* leaf_prims, long cap_prims) {
  if (!sb) return GLOME_E_INVALID;
  try {
    const Node& n = sb->graph.at(id);
    if (n.kind != K_BIH) throw std::invalid_argument("not a Bih");
    const BihTree& T = *n.bih;
    long cnt = 0, np = 0;
    std::vector<int> st{0};
    while (!st.empty()) {  // preorder, left before right
      const BihTree::Node& bn = T.nodes[st.back()];
      st.pop_back();
      if (cnt < cap) {
        axis[cnt] = bn.leaf ? -1 : bn.axis; nleaf[cnt] = bn.leaf ? (int)bn.items.size() : 0;
        lsplit[cnt] = bn.leaf ? 0 : bn.lsplit; rsplit[cnt] = bn.leaf ? 0 : bn.rsplit;
      }
      cnt++;
      if (bn.leaf) { for (int it : bn.items) { if (np < cap_prims) leaf_prims[np] = it; np++; } }
      else { st.push_back(bn.right); st.push_back(bn.left); }
    }
    return cnt;
  } catch (const std::exception& e) { sb->err = e.what(); return GLOME_E_INVALID; }
}

int glome_tiles_layout(const glome_render_params* P, int tile_first, int tile_stride, int32_t* xywh_base, int cap) {
  if (!P || P->width <= 0 || P->height <= 0 || P->blocksize <= 0 || tile_stride <= 0 || tile_first < 0) return GLOME_E_INVALID;
  std::vector<DTile> t; uint32_t w; int64_t px;
  owned_tiles(P->width, P->height, P->blocksize, tile_first, tile_stride, P->rank0_share_pct, t, w, px);
  for (size_t k = 0; k < t.size() && (int)k < cap; k++) {
    xywh_base[5 * k] = t[k].x; xywh_base[5 * k + 1] = t[k].y; xywh_base[5 * k + 2] = t[k].w; xywh_base[5 * k + 3] = t[k].h; xywh_base[5 * k + 4] = (int32_t)t[k].pix_base;
  }
  return (int)t.size();
}

int64_t glome_items_layout(const glome_render_params* P, int tile_first, int tile_stride, int blocksize_override, int which, int32_t* out, int64_t cap_items) {
  if (!P || P->width <= 0 || P->height <= 0 || P->blocksize <= 0 || tile_stride <= 0 || tile_first < 0 || blocksize_override < 0) return GLOME_E_INVALID;
  std::vector<DTile> t; uint32_t total; int64_t px;
  owned_tiles(P->width, P->height, blocksize_override ? blocksize_override : P->blocksize, tile_first, tile_stride, P->rank0_share_pct, t, total, px);
  std::vector<DItem> items;
  if (which) build_item_table(t, total, items);
  size_t tile = 0;
  for (uint32_t w = 0; w < total && (int64_t)w < cap_items; w++) {
    while (tile + 1 < t.size() && t[tile + 1].wave_base <= w) tile++;
    for (int lane = 0; lane < 64; lane++) {
      int x = 0, y = 0; size_t off = 0;
      const bool valid = which ? item_pixel(items[w], t.data(), lane, x, y, off) : tile_item_pixel(t[tile], w - t[tile].wave_base, lane, x, y, off);
      int32_t* o = out + ((size_t)w * 64 + lane) * 4;
      o[0] = valid ? 1 : 0; o[1] = valid ? x : 0; o[2] = valid ? y : 0; o[3] = valid ? (int32_t)off : 0;
    }
  }
  return (int64_t)total;
}

// ---- the choice of a kernel instance, seen from the host (instances.hpp) ----
static_assert(all_choices_listed(std::make_integer_sequence<int, 128>{}), "a choice rule names a kernel instance that no X-list holds");

int64_t glome_kernel_choice(int64_t n, const int64_t* in, int32_t* out) {
  if (n < 0 || (n > 0 && (!in || !out))) return GLOME_E_INVALID;
  for (int64_t i = 0; i < n; i++) {
    const int64_t* v = in + 14 * i;
    SceneTraits s;
    s.tier = (int)v[0]; s.cls_mask = (int)v[1]; s.has_secondary_mats = v[2] != 0; s.has_nested_mats = v[3] != 0; s.has_refract = v[4] != 0; s.pk_all = v[5] != 0;
    s.stack_cap = (int)v[6]; s.n_bih_nodes = v[7];
    if (v[8] != GLOME_MODE_TILE && v[8] != GLOME_MODE_SUBSAMPLE) return GLOME_E_INVALID;
    const bool sampler = v[8] == GLOME_MODE_SUBSAMPLE;
    const Choice c = sampler ? choose_sampler(s, v[9] != 0, v[10] != 0, (int)v[11], (int)v[12]) : choose_render(s, v[9] != 0, v[10] != 0, (int)v[11], (int)v[12], (uint32_t)v[13]);
    int32_t* o = out + 4 * i;
    o[0] = sampler ? KIND_SAMPLER : KIND_RENDER; o[1] = c.generic ? (c.generic_counts ? -1 : -2) : c.key; o[2] = c.two_rows ? 1 : 0; o[3] = waves_per_cu(c);
  }
  return n;
}
int64_t glome_trace_kernel_choice(int64_t n, const int64_t* in, int32_t* out) {
  if (n < 0 || (n > 0 && (!in || !out))) return GLOME_E_INVALID;
  for (int64_t i = 0; i < n; i++) {
    const int64_t* v = in + 11 * i;
    SceneTraits s;
    s.tier = (int)v[0]; s.cls_mask = (int)v[1]; s.has_secondary_mats = v[2] != 0; s.has_nested_mats = v[3] != 0; s.has_refract = v[4] != 0; s.pk_all = v[5] != 0;
    s.stack_cap = (int)v[6]; s.n_bih_nodes = v[7];
    const Choice c = choose_trace(s, v[8] != 0, v[9] != 0, (int)v[10]);
    int32_t* o = out + 3 * i;
    o[0] = c.generic ? (c.generic_counts ? -1 : -2) : c.key; o[1] = c.lb; o[2] = waves_per_cu(c);
  }
  return n;
}
int glome_sb_scene_traits(glome_sb* sb, int32_t root, int64_t* out) {
  if (!sb || !out) return GLOME_E_INVALID;
  try {
    FlatScene F;
    Flattener fl(sb_graph(sb), F);
    fl.run(root);
    const CommitRules R = commit_rules(sb_graph(sb), F);
    const SceneTraits& t = R.traits;
    const int64_t v[11] = {t.tier, t.cls_mask, t.has_secondary_mats, t.has_nested_mats, t.has_refract, t.pk_all, t.stack_cap, t.n_bih_nodes, R.caps.ovf_cap, R.caps.pk_generic_cap, t.n_mesh_nodes};
    memcpy(out, v, sizeof(v));
    return 0;
  } catch (const std::exception& e) { sb->err = e.what(); return GLOME_E_INVALID; }
}

}  // extern "C"
