// flatten.hpp -- turn the host scene graph (host_graph.hpp) into the packed pools of rt_types.h.
// This is the "Haskell host flattens the scene graph to packed SoA device buffers" step; it is pure host
// code (no HIP) so the layout can be inspected and tested without a GPU.
#pragma once
#include <limits>
#include <cstring>
#include <functional>
#include <map>
#include <set>
#include <unordered_map>

#include "host_graph.hpp"
#include "rt_types.h"

namespace glome {

// What an update of a committed Mesh's vertices needs (glome_scene_mesh_update; mesh_update_kernels.hpp), recorded per emitted mesh and
// kept beside the scene, outside DScene.  Record j of the mesh is mtris record first_tri + j; its index row is rows[8 j ..]:
// a b c na nb nc, the triangle's first trinorms word or -1, a spare word.  The placeholder record of an empty leaf has a = -1.
// The second answer of mark_updatable, per Mesh, triangle bih and Instance: whether an update is accepted when the bihs above the object
// are refitted after it (glome_scene_nested_updates, glome_scene_bih_refit), and those bihs in an order in which they can be refitted --
// a tree after every tree below it.  `plain` stays what it was: the answer with the switch off.  Both answers have one shape: whether,
// and if not the reason.
struct UpdateAnswer {
  bool ok = true;
  std::string why_not;
};
struct NestedAnswer : UpdateAnswer {
  std::vector<int> above;
};

struct MeshUpdateInfo {
  int node = -1;                  // the mesh's builder id
  int nv = 0, nn = 0;
  uint32_t hdr = 0;               // meshhdr index
  uint32_t first_node = 0, n_nodes = 0;  // its branch nodes (meshnodes index, count)
  uint32_t first_tri = 0, n_tris = 0;    // its mtris records (placeholders included)
  std::vector<int32_t> rows;
  std::vector<uint32_t> level_nodes;  // its branch nodes, deepest tree level first ...
  std::vector<uint32_t> level_off;    // ... level l is level_nodes[level_off[l] .. level_off[l + 1])
  UpdateAnswer plain;             // not ok: a path from the committed root to the mesh passes through a Bih, whose planes and root box were
                                  // built from the mesh's bound (Bih.hs:309-324) -- the reason, naming that bih
  NestedAnswer nested;            // the answer with glome_scene_nested_updates on (Flattener::mark_nested)
  double bound6[6] = {0, 0, 0, 0, 0, 0};  // bound(mesh) at commit: lo, hi
};

// What an update of a committed leaf bih's items needs -- a triangle bih's triangles (glome_scene_bih_update; bih_update_kernels.hpp) or a
// sphere bih's spheres (glome_scene_sphere_bih_update; sphere_bih_update_kernels.hpp) -- recorded per emitted bih of class BC_TRI or
// BC_SPHERE and kept beside the scene, outside DScene.  The tree's leaves are emitted in preorder with nothing in between, so record j of
// the tree is `recs` record first_rec + j and `tris` / `spheres` record first_prim + j.  A row is row_words words.  A sphere's is its
// item (its index in BihTree::update_order).  A triangle's is its item, then where its words go in `tripairs`: the pair record's first
// word (a float index), kPairHalfB when it is the record's second triangle, kPairBoth when it is an odd last one that is paired with
// itself; kNoPair when the tree has no packet form.  A branch's two child references are read from its node, whose .zw words an update
// never writes.  A sphere tree has no packet node copy: its walk reads bihnodes.
struct LeafBihUpdateInfo {
  static constexpr uint32_t kPairHalfB = 1u << 29, kPairBoth = 1u << 30, kNoPair = 0xffffffffu;
  int node = -1;                  // the bih's builder id
  uint32_t cls = BC_TRI;          // BC_TRI or BC_SPHERE
  int n_items = 0;
  uint32_t hdr = 0;               // bihhdr index
  uint32_t first_slot = 0, n_slots = 0;  // its node slots (bihnodes index, count; unused slots included)
  uint32_t first_prim = 0, first_rec = 0, n_recs = 0;
  uint32_t n_pair_recs = 0;       // its pair records in `tripairs` (LeafBihLayout::n_pair_recs) ...
  uint64_t first_pair_word = 0;   // ... from this float index on
  int depth = 0;                  // BihTree::depth
  uint32_t row_words = 2;         // 2 for triangles, 1 for spheres
  bool pk = false;                // the tree has the packet form: pknodes and tripairs follow (never a sphere tree)
  std::vector<uint32_t> rows;
  std::vector<uint32_t> level_nodes;  // its branch slots (bihnodes indices), deepest tree level first ...
  std::vector<uint32_t> level_off;    // ... level l is level_nodes[level_off[l] .. level_off[l + 1])
  UpdateAnswer plain;             // not ok: another Bih lies above it, or the scene holds another copy of one of its items -- the reason
  NestedAnswer nested;
  double bound6[6] = {0, 0, 0, 0, 0, 0};  // bound(bih) at commit
  const char* item_word() const { return cls == BC_SPHERE ? "sphere" : "triangle"; }
};

// What an update of committed Instances' matrices needs (glome_scene_instance_update; instance_update_kernels.hpp), kept beside the
// scene, outside DScene.  Per emitted Instance node: its slots in the `xfms` pool (emit memoises a node's record, so today a node has
// exactly one however many parents hold it; the list is what the update walks), and -- when it is an item of a bih -- which bih and which
// of that bih's items.
struct InstanceUpdateInfo {
  int node = -1;                  // the Instance's builder id
  std::vector<uint32_t> slots;    // xfm indices (six float4 each)
  int bih = -1;                   // the bih it is an item of (builder id), -1: of none
  uint32_t item = 0;              // ... and its item there (an index into InstBihInfo's per-item arrays)
  UpdateAnswer plain;             // not ok: see Flattener::mark_updatable -- the reason
  NestedAnswer nested;
};
// Per emitted bih, of class BC_CSG or BC_GENERIC (no other class can hold one), with at least one Instance item or one LIVE item: an
// item that, Tex / Tag / shadow wrappers peeled off, is a Mesh or a Bih (a direct item) or an Instance of one under wrappers (an
// instanced item) -- what glome_scene_bih_refit makes again from the object's fp64 bound.  Its items are its leaf
// records in emission order; item j's record is recs[first_rec + rec_off[j]] -- the leaves' runs are NOT adjacent here: an item's own
// records (an Instance's child slot, a list's members) lie between them.  rows: per item two fp32 boxes as the host derives them from the
// fp64 bound(item) -- the plane form, round_down((lo - kDelta)) / round_up((hi + kDelta)) (a branch's plane is one more pad beyond the
// item's box; bih_update_kernels.hpp plane_add), then the box form, round_down(lo) / round_up(hi) (what the header's box is the fold of):
// four F4 per item, (plane lo, plane hi, box lo, box hi).  child_bound: per item the six doubles of bound(child) when the item is an
// Instance (lo, hi), zeros otherwise.  kind / live / box64 / live_xf: the tables of a refit -- per item its kind and the builder id of
// the object it hangs on (-1: none), the six doubles of bound(item) at commit, and for the instanced items, in item order, the 24 doubles
// of the Instance's matrix at commit (xf_at: which row).  An item over a Bih the scene cannot update (boxes, say) counts as static.
struct InstBihInfo {
  enum ItemKind : uint8_t { kStatic = 0, kInstance = 1, kDirectLive = 2, kInstancedLive = 3 };
  std::vector<uint8_t> kind;
  std::vector<int> live;
  std::vector<double> box64, live_xf;
  std::vector<int32_t> xf_at;     // per item: its row of live_xf, -1: none
  NestedAnswer nested;            // of the bih itself, as a live object of the trees above it: ok = every tree above can be refitted after it
  double bound6[6] = {0, 0, 0, 0, 0, 0};  // bound(bih) at commit
  int node = -1;                  // the bih's builder id
  uint32_t hdr = 0;               // bihhdr index
  uint32_t first_slot = 0, n_slots = 0;  // its node slots (bihnodes index, count)
  uint32_t first_rec = 0, rec_span = 0;  // its leaf records lie in recs[first_rec .. first_rec + rec_span)
  std::vector<uint32_t> rec_off;
  std::vector<F4> rows;
  std::vector<double> child_bound;
  std::vector<uint32_t> level_nodes;  // its branch slots (bihnodes indices), deepest tree level first ...
  std::vector<uint32_t> level_off;    // ... level l is level_nodes[level_off[l] .. level_off[l + 1])
};

struct FlatScene {
  std::vector<U4> recs;
  std::vector<F4> spheres, tris, trinorms, boxes, planes, discs, quadrics, xfms, bihhdr, bihnodes, meshhdr, meshnodes, mtris, mats, wlights;
  std::vector<U4> mtrimeta, entries;
  std::vector<U4> walk;  // the walk-entry table: one record per entry of `entries` (emit_walk; rt_types.h DScene::walk)
  std::vector<uint32_t> matkids;
  std::vector<float> tripairs;  // the pair records of the triangle BIHs' leaves (emit_pairs; bih_packet_asm.hpp)
  std::vector<F4> pknodes;      // the packet walk's copy of the triangle BIHs' branch nodes: same slots as bihnodes, child references in its own form
  uint32_t root_rec = 0;
  uint32_t tier = 1;
  int nesting_depth = 0, max_bih_depth = 0, max_mesh_depth = 0;
  int vm_words = 0;  // the frame words run() estimated for a ray of this scene: what it held against kVmWords (host side only: tests)
  int max_sphere_bih_depth = 0;  // deepest BIH the interpreter's packet service can walk: items all plain spheres, all plain triangles, or all answered in place (0: none)
  uint32_t tex_bits = 16;   // bits per id of a TexStack (rt_types.h): 8 when the scene has at most 254 materials
  int64_t n_other_prims = 0;
  std::string why_generic;  // why the flat tier was not chosen
  bool pk_all = true;       // every triangle BIH has the packet walk's node form (emit_bih); the trait of the same name asks for more (capi_shared.hpp commit_rules)
  std::vector<MeshUpdateInfo> mesh_updates;  // one per emitted mesh (emit_mesh), in emission order
  std::vector<LeafBihUpdateInfo> leaf_bih_updates;  // one per emitted triangle or sphere bih (emit_bih), in emission order
  std::vector<InstanceUpdateInfo> inst_updates;  // one per emitted Instance node (emit), in emission order
  std::vector<InstBihInfo> inst_bihs;        // one per emitted bih that holds an Instance as an item (emit_bih), in emission order
};

inline float f32(double d) { return (float)d; }
inline float as_float_bits(uint32_t u) { float f; std::memcpy(&f, &u, 4); return f; }
inline F4 mk4(double x, double y, double z, double w) { return F4{f32(x), f32(y), f32(z), f32(w)}; }
inline F4 mk4u(double x, double y, double z, uint32_t w) { return F4{f32(x), f32(y), f32(z), as_float_bits(w)}; }
// split planes are rounded outward so that an fp32 plane never cuts into the objects it bounds
// (host and device: the mesh update's kernels round with these very functions, mesh_update_kernels.hpp)
GLOME_HD float round_up(double d) { float f = (float)d; return ((double)f < d) ? nextafterf(f, INFINITY) : f; }
GLOME_HD float round_down(double d) { float f = (float)d; return ((double)f > d) ? nextafterf(f, -INFINITY) : f; }

constexpr uint32_t BREF_LEAF_BIT = 1u << 29, BREF_FIRST_LIMIT = 1u << 26;  // child references, see rt_device.hpp

// Node slots of a committed bih: only branches (and leaves of 7+ items, whose extent lives in a slot) get one.  Branches are laid out
// in small treelets -- a node, then its branch children, then a grandchild, four 16-byte nodes to a 64-byte cache
// line -- and the treelets depth first, so the step after a fetch usually finds its node in the line just fetched
// and a subtree is contiguous.  References are explicit, so the traversal does not care about the order.
// slot[k]: node k's slot from the tree's (line-aligned) base, 0xffffffff for none; returns the slots used, skipped ones included.
inline uint32_t bih_slots(const BihTree& T, std::vector<uint32_t>& slot) {
  slot.assign(T.nodes.size(), 0xffffffffu);
  uint32_t nslots = 0;
  std::vector<int> roots;  // treelet roots still to place (a stack: depth first)
  if (!T.nodes.empty() && !T.nodes[0].leaf) roots.push_back(0);
  while (!roots.empty()) {
    int x = roots.back(); roots.pop_back();
    int group[4]; int ng = 0;
    group[ng++] = x;
    for (int q = 0; q < ng && ng < 4; q++) {  // breadth first inside the treelet
      const BihTree::Node& b = T.nodes[group[q]];
      if (!T.nodes[b.left].leaf && ng < 4) group[ng++] = b.left;
      if (!T.nodes[b.right].leaf && ng < 4) group[ng++] = b.right;
    }
    // a treelet never straddles a cache line: one that would is started on the next line (the skipped slots stay unused)
    if ((nslots & 3u) + (uint32_t)ng > 4u) nslots = (nslots + 3u) & ~3u;
    for (int q = 0; q < ng; q++) slot[group[q]] = nslots++;
    // branch children of the group's members that did not fit start treelets of their own; right pushed first so the
    // left subtree is laid out next
    for (int q = ng - 1; q >= 0; q--) {
      const BihTree::Node& b = T.nodes[group[q]];
      if (!T.nodes[b.right].leaf && slot[b.right] == 0xffffffffu) roots.push_back(b.right);
      if (!T.nodes[b.left].leaf && slot[b.left] == 0xffffffffu) roots.push_back(b.left);
    }
  }
  for (size_t k = 0; k < T.nodes.size(); k++) if (T.nodes[k].leaf && T.nodes[k].items.size() > 6) slot[k] = nslots++;
  return nslots;
}

// A tree's branch nodes by tree level, deepest first (a level's children were refitted by the launch before it): what the Mesh's update
// launches k_mesh_refit_level over, and the triangle bih's update and an item bih's refit k_bih_level.  `nodes`: a BihTree's or a
// MeshData's, each with leaf / left / right; stored(k): where node k lies in its pool.  Nothing for a tree whose root is a leaf.
template <class Nodes, class Stored>
inline void tree_levels(const Nodes& nodes, Stored stored, std::vector<uint32_t>& level_nodes, std::vector<uint32_t>& level_off) {
  if (nodes.empty() || nodes[0].leaf) return;
  std::vector<int> depth(nodes.size(), 0), order{0};  // (a parent before its children, whatever the numbering)
  for (size_t q = 0; q < order.size(); q++) {
    const auto& bn = nodes[(size_t)order[q]];
    if (bn.leaf) continue;
    for (int c : {bn.left, bn.right}) { depth[(size_t)c] = depth[(size_t)order[q]] + 1; order.push_back(c); }
  }
  int deepest = 0;
  for (int k : order) if (!nodes[(size_t)k].leaf) deepest = std::max(deepest, depth[(size_t)k]);
  std::vector<uint32_t> per_level((size_t)deepest + 2, 0);
  for (int k : order) if (!nodes[(size_t)k].leaf) per_level[(size_t)(deepest - depth[(size_t)k]) + 1]++;
  for (size_t l = 1; l < per_level.size(); l++) per_level[l] += per_level[l - 1];
  level_off = per_level;
  level_nodes.resize(per_level.back());
  std::vector<uint32_t> fill(per_level.begin(), per_level.end() - 1);
  for (int k : order) if (!nodes[(size_t)k].leaf) level_nodes[fill[(size_t)(deepest - depth[(size_t)k])]++] = stored((size_t)k);
}

// The topology half of a committed triangle or sphere bih (class BC_TRI / BC_SPHERE): everything Flattener::emit_bih lays out for the
// tree that depends on its shape and on where its segments start, and on no coordinate -- so that a commit and a rebuild of the tree in a
// committed scene (glome_sb_bih_layout reports its sizes) lay the same tree out alike.  The tree's leaves are emitted in preorder with
// nothing in between: record j of the tree is recs[first_rec + j] and tris / spheres[first_prim + j], and a triangle tree's pair records
// follow one another from float index first_pair_word of `tripairs`.  item_of[i]: the index of leaf item i in the update order.
struct LeafBihLayout {
  uint32_t base = 0, n_slots = 0;     // the node slots: bihnodes / pknodes [base, base + max(n_slots, 1))
  uint32_t first_rec = 0, first_prim = 0, n_recs = 0;
  uint64_t first_pair_word = 0;
  uint32_t n_pair_recs = 0;           // pair records laid out (a tree that gives the packet form up part way keeps the ones before)
  bool pk = false;                    // the tree has the packet form
  int depth = 0;
  std::vector<uint32_t> slot;         // per tree node (bih_slots)
  std::vector<uint32_t> ref;          // per tree node: the reference a parent (ref[0]: the header) holds (rt_device.hpp BREF_*)
  std::vector<uint32_t> pkleaf;       // per tree node, a leaf as the packet walk refers to it: byte offset of its first pair record | 3
  std::vector<uint32_t> leaf_first;   // per tree node, a leaf's first record as an offset from first_rec
  std::vector<uint8_t> paired;        // per tree node: the leaf has pair records
  std::vector<uint32_t> pair_words;   // per pair record: the count word and the record-index word (emit_pairs)
  std::vector<uint32_t> node_zw;      // per slot: words .z .w of the bihnodes entry (a branch's child references; a slot leaf's count and first record)
  std::vector<uint32_t> pk_zw;        // per slot: words .z .w of the pknodes entry (branches of a tree that has the packet form)
  std::vector<uint32_t> rows;         // LeafBihUpdateInfo::rows
  std::vector<uint32_t> level_nodes, level_off;  // LeafBihUpdateInfo's
  uint32_t hdr2[4] = {0, 0, 0, 0};    // bihhdr[3 h + 2]: records-to-pool delta, packet root, packet flag, depth
};
inline LeafBihLayout leaf_bih_layout(const BihTree& T, uint32_t cls, const std::vector<uint32_t>& item_of, uint32_t base, uint32_t first_rec, uint32_t first_prim,
                                     uint64_t first_pair_word) {
  constexpr uint32_t kPairHalfB = 1u << 29, kPairBoth = 1u << 30, kNoPair = 0xffffffffu;  // (LeafBihUpdateInfo's)
  LeafBihLayout L;
  L.base = base; L.first_rec = first_rec; L.first_prim = first_prim; L.first_pair_word = first_pair_word; L.depth = T.depth;
  L.n_slots = bih_slots(T, L.slot);
  if (base + L.n_slots >= BREF_FIRST_LIMIT) throw limit_error("too many BIH nodes");
  bool pk = cls == BC_TRI && base + L.n_slots < (1u << 27);  // (a node's byte offset is a reference: 31 bits)
  const size_t nn = T.nodes.size();
  L.ref.assign(nn, 0); L.pkleaf.assign(nn, 3u); L.leaf_first.assign(nn, 0); L.paired.assign(nn, 0);
  L.node_zw.assign(2 * (size_t)std::max<uint32_t>(L.n_slots, 1u), 0); L.pk_zw = L.node_zw;
  uint64_t pair_at = first_pair_word;  // (a float index)
  for (size_t k = 0; k < nn; k++) {
    const BihTree::Node& bn = T.nodes[k];
    if (!bn.leaf) { L.ref[k] = base + L.slot[k]; continue; }
    const uint32_t count = (uint32_t)bn.items.size(), leaf_rec = first_rec + L.n_recs;
    L.leaf_first[k] = L.n_recs;
    if ((uint64_t)leaf_rec + count >= BREF_FIRST_LIMIT) throw limit_error("too many records for the BIH leaf references");
    bool paired = false;
    if (cls == BC_TRI && count && pk) {
      if ((pair_at + (uint64_t)count * kPairWords) * 4 >= (1ull << 31)) pk = false;  // (a pair record's byte offset is a reference)
      else {
        L.pkleaf[k] = (uint32_t)(pair_at * 4u) | 3u; paired = true;
        for (uint32_t j = 0; j < count; j += 2) { L.pair_words.push_back(count - j); L.pair_words.push_back(leaf_rec + j); }
        pair_at += (uint64_t)((count + 1u) / 2u) * kPairWords;
      }
    }
    L.paired[k] = paired;
    for (uint32_t q = 0; q < count; q++) {
      L.rows.push_back(item_of[(size_t)bn.items[q]]);
      if (cls != BC_TRI) continue;
      const uint32_t pair = (L.pkleaf[k] & ~3u) / 4u + (q / 2u) * kPairWords;  // (a float index: below 2^29)
      L.rows.push_back(!paired ? kNoPair : (pair | (q & 1u ? kPairHalfB : 0u) | (q + 1 == count && !(q & 1u) ? kPairBoth : 0u)));
    }
    if (count == 0) L.ref[k] = BREF_LEAF_BIT;
    else if (count <= 6) L.ref[k] = BREF_LEAF_BIT | (count << 26) | leaf_rec;
    else {
      L.node_zw[2 * (size_t)L.slot[k]] = count; L.node_zw[2 * (size_t)L.slot[k] + 1] = leaf_rec;
      L.ref[k] = BREF_LEAF_BIT | (7u << 26) | (base + L.slot[k]);
    }
    L.n_recs += count;
  }
  L.pk = pk;
  L.n_pair_recs = (uint32_t)(L.pair_words.size() / 2);
  for (size_t k = 0; k < nn; k++) {
    const BihTree::Node& bn = T.nodes[k];
    if (bn.leaf) continue;
    L.node_zw[2 * (size_t)L.slot[k]] = (uint32_t)bn.axis | (L.ref[bn.left] << 2); L.node_zw[2 * (size_t)L.slot[k] + 1] = L.ref[bn.right];
    // The hand-written packet walk (bih_packet_asm.hpp) reads its own copy: a branch child is referred to by its BYTE OFFSET
    // in this pool with the child's axis in the two low bits (scalar loads ignore them), a leaf child by the byte offset of
    // its first pair record (tripairs) with both low bits set -- the step's code is picked, the near child's node asked for
    // and a leaf's triangles fetched without a shift, a mask or a multiplication.  (An empty leaf is 3: never entered.)
    if (pk) {
      auto pkref = [&](int c) { return T.nodes[c].leaf ? L.pkleaf[c] : (((base + L.slot[c]) << 4) | (uint32_t)T.nodes[c].axis); };
      L.pk_zw[2 * (size_t)L.slot[k]] = pkref(bn.left); L.pk_zw[2 * (size_t)L.slot[k] + 1] = pkref(bn.right);
    }
  }
  if (cls == BC_TRI && !pk) for (size_t j = 0; j < L.n_recs; j++) L.rows[2 * j + 1] = kNoPair;  // (the packet form was given up part way)
  tree_levels(T.nodes, [&](size_t k) { return base + L.slot[k]; }, L.level_nodes, L.level_off);
  // (y: the root in the packet walk's form, z: 1 when this tree has that form -- triangle leaves, byte offsets that fit a reference;
  // w: the tree's depth -- a leaf class never has kBihItemsInPlace, its trees have packet walks of their own)
  const uint32_t pkroot = (pk && !T.nodes.empty() && !T.nodes[0].leaf) ? (((base + L.slot[0]) << 4) | (uint32_t)T.nodes[0].axis) : 0u;
  L.hdr2[0] = L.n_recs ? first_prim - first_rec : 0u; L.hdr2[1] = pkroot; L.hdr2[2] = pk ? 1u : 0u; L.hdr2[3] = (uint32_t)T.depth;
  return L;
}

class Flattener {
 public:
  Flattener(const Graph& g, FlatScene& out) : G(g), F(out) {}

  void run(int root) {
    emit_materials();
    // generic representation: always built (the per-ray batch seams and the generic tier use it)
    U4 r = emit(root);
    F.root_rec = (uint32_t)F.recs.size();
    F.recs.push_back(r);
    F.nesting_depth = depth_of(root);
    F.tex_bits = G.mats.size() <= 254 ? 8 : 16;
    tex_cap = 64 / (int)F.tex_bits;
    if (tex_depth_of(root) > tex_cap)
      throw limit_error("a primitive lies under " + std::to_string(tex_depth_of(root)) + " nested textures; the device's texture stack holds " + std::to_string(tex_cap) +
                        (tex_cap < kMaxTexDepth ? " in a scene of more than 254 materials (" + std::to_string(kMaxTexDepth) + " otherwise)" : ""));
    const bool warps = bind_warps();  // Warp materials refer to records: the frame's, and the scene's they look into
    F.vm_words = std::max(vm_words_of(root) + 2, warp_words);
    if (F.vm_words > kVmWords)
      throw limit_error("scene nests deeper than the device interpreter's frame memory holds (" + std::to_string(F.vm_words) + " of " + std::to_string(kVmWords) + " words)");
    // flat tier: root program of simple entries
    F.tier = 0;
    if (warps) { F.tier = 1; F.why_generic = "a Warp material traces other roots than the scene's"; }
    collect_entries(root, 0, 0, 0);
    if (F.tier == 0 && F.max_bih_depth > kFlatStack) { F.tier = 1; F.why_generic = "BIH deeper than the LDS stack"; }
    if (F.tier == 0 && F.max_mesh_depth > kFlatStack) { F.tier = 1; F.why_generic = "Mesh BVH deeper than the LDS stack"; }
    if (F.tier != 0) F.entries.clear();
    // the generic tier walks BIHs / Mesh BVHs with a fixed scratch stack per level: a deeper tree is refused, not truncated
    if (F.tier != 0 && F.max_mesh_depth > kGenericStack)
      throw limit_error("Mesh tree deeper than the device traversal stack (" + std::to_string(F.max_mesh_depth) + " > " + std::to_string(kGenericStack) + ")");
    mark_updatable(root);
    mark_nested(root);
    pad();
    emit_walk();
  }

 private:
  const Graph& G;
  FlatScene& F;
  std::unordered_map<int, U4> memo;  // host node id -> record value (shared subtrees are emitted once)

  static bool is_prim(int k) { return k >= K_SPHERE && k <= K_CONE; }

  // The packet walk tests a leaf's triangles two at a time.  A leaf of n triangles owns ceil(n / 2) consecutive PAIR RECORDS of
  // kPairWords words: every component of p1, e1, e2 of triangles 2j and 2j + 1 as an (A, B) pair -- p1x p1y p1z e1x e1y e1z e2x
  // e2y e2z, 18 floats -- then the number of the leaf's triangles from 2j on (what the walk's loop counts down) and the record
  // index of triangle 2j (what a hit reports).  An odd last triangle is paired with itself; the walk ignores that half.
  uint32_t emit_pairs(uint32_t first_prim, uint32_t count, const uint32_t* words) {  // words: the layout's two per record (LeafBihLayout::pair_words)
    const uint32_t at = (uint32_t)F.tripairs.size();
    for (uint32_t j = 0; j < count; j += 2) {
      const size_t a = first_prim + j, b = j + 1 < count ? a + 1 : a;
      float r[kPairWords];
      for (int w = 0; w < 3; w++) {  // word w of a triangle record: (p1, .) (e1, .) (e2, .)
        const F4 &A = F.tris[3 * a + w], &B = F.tris[3 * b + w];
        r[6 * w + 0] = A.x; r[6 * w + 1] = B.x; r[6 * w + 2] = A.y; r[6 * w + 3] = B.y; r[6 * w + 4] = A.z; r[6 * w + 5] = B.z;
      }
      r[18] = as_float_bits(words[j]);  // (two words per record, a record per two triangles: record j / 2's are words[j], words[j + 1])
      r[19] = as_float_bits(words[j + 1]);
      F.tripairs.insert(F.tripairs.end(), r, r + kPairWords);
    }
    return at * 4u;  // byte offset of the leaf's first record
  }

  // The walk-entry table (rt_types.h DScene::walk): per entry the words the entry loops read from `entries` and `recs` before a walk
  // starts.  Every scene gets one, the padding entry of a scene without a root program included; only the flagship render instance and its
  // cull pass read it.  After pad(): one record per entry as the device sees them.
  void emit_walk() {
    F.walk.clear();
    for (const U4& e : F.entries) {
      const U4& r = F.recs[e.x];
      F.walk.push_back(U4{e.z, r.y, e.y, r.x});
    }
  }

  void pad() {  // never hand a null pool to a kernel
    auto p4 = [](std::vector<F4>& v) { if (v.empty()) v.push_back(F4{0, 0, 0, 0}); };
    p4(F.spheres); p4(F.tris); p4(F.trinorms); p4(F.boxes); p4(F.planes); p4(F.discs); p4(F.quadrics); p4(F.xfms);
    p4(F.bihhdr); p4(F.bihnodes); p4(F.meshhdr); p4(F.meshnodes); p4(F.mtris); p4(F.mats); p4(F.wlights);
    if (F.mtrimeta.empty()) F.mtrimeta.push_back(U4{0, 0, 0, 0});
    if (F.entries.empty()) F.entries.push_back(U4{0, 0, 0, 0});
    if (F.matkids.empty()) F.matkids.push_back(0);
    if (F.tripairs.empty()) F.tripairs.assign(kPairWords, 0.0f);
    if (F.pknodes.size() < F.bihnodes.size()) F.pknodes.resize(F.bihnodes.size(), F4{0, 0, 0, 0});
  }

  void emit_materials() {
    for (const Mat& m : G.mats) {
      uint32_t a = 0, b = 0;
      F4 m1{0, 0, 0, 0}, m2{0, 0, 0, 0};
      float w = 0;
      switch (m.kind) {
        case MAT_SURFACE: m1 = mk4(m.color[0], m.color[1], m.color[2], m.alpha); m2 = mk4(m.amb, m.kd, m.ks, m.shine); break;
        case MAT_REFLECT: m1 = mk4(m.refl, 0, 0, 0); break;
        case MAT_REFRACT: m1 = mk4(m.refl, m.refr, m.ior, 0); break;
        case MAT_LAYERS: a = (uint32_t)F.matkids.size(); b = (uint32_t)m.kids.size(); for (int k : m.kids) F.matkids.push_back((uint32_t)k); break;
        case MAT_BLEND:
          a = (uint32_t)m.a; b = (uint32_t)m.b; w = f32(m.weight);
          m1 = F4{as_float_bits((uint32_t)m.wfn), f32(m.wp[0]), f32(m.wp[1]), f32(m.wp[2])};  // weight function + parameters
          break;
        case MAT_WARP: break;  // filled in by bind_warps once the records exist
      }
      F.mats.push_back(F4{as_float_bits((uint32_t)m.kind), as_float_bits(a), as_float_bits(b), w});
      F.mats.push_back(m1);
      F.mats.push_back(m2);
    }
    if (mat_nest_max() > kMaxMatNest) throw limit_error("material Blend/AdditiveLayers nesting deeper than the device shader supports");
    if (G.mats.size() > 65534) throw limit_error("more than 65534 materials");
  }
  // Warp materials: (kind, frame record, scene record, transform) (first light, light count, -, -)
  bool bind_warps() {
    bool any = false;
    for (size_t k = 0; k < G.mats.size(); k++) {
      const Mat& m = G.mats[k];
      if (m.kind != MAT_WARP) continue;
      any = true;
      const uint32_t frame = slot(emit(m.wframe)), scene = m.wscene < 0 ? F.root_rec : slot(emit(m.wscene));
      F.nesting_depth = std::max(F.nesting_depth, std::max(depth_of(m.wframe), m.wscene < 0 ? 0 : depth_of(m.wscene)));
      if (std::max(tex_depth_of(m.wframe), m.wscene < 0 ? 0 : tex_depth_of(m.wscene)) > tex_cap) throw limit_error("a Warp material's frame / scene has more nested textures than the device's texture stack holds");
      // (the shader traces these roots from an empty frame memory, like the scene's own: the same estimate, and the largest goes to FlatScene::vm_words)
      warp_words = std::max(warp_words, std::max(vm_words_of(m.wframe), m.wscene < 0 ? 0 : vm_words_of(m.wscene)) + 2);
      if (warp_words > kVmWords)
        throw limit_error("a Warp material's frame / scene nests deeper than the device interpreter's frame memory holds (" + std::to_string(warp_words) + " of " + std::to_string(kVmWords) + " words)");
      const uint32_t xf = (uint32_t)(F.xfms.size() / 6);
      for (int q = 0; q < 3; q++) F.xfms.push_back(mk4(m.wxf.f.m[4 * q], m.wxf.f.m[4 * q + 1], m.wxf.f.m[4 * q + 2], m.wxf.f.m[4 * q + 3]));
      for (int q = 0; q < 3; q++) F.xfms.push_back(mk4(m.wxf.i.m[4 * q], m.wxf.i.m[4 * q + 1], m.wxf.i.m[4 * q + 2], m.wxf.i.m[4 * q + 3]));
      const uint32_t first = (uint32_t)(F.wlights.size() / 2);
      for (const WarpLight& L : m.wlights) {  // the layout of DLight: pos, color, rad, shadow
        F.wlights.push_back(mk4(L.pos[0], L.pos[1], L.pos[2], L.color[0]));
        F.wlights.push_back(F4{f32(L.color[1]), f32(L.color[2]), f32(L.rad), as_float_bits(L.shadow ? 1u : 0u)});
      }
      F.mats[3 * k] = F4{as_float_bits((uint32_t)MAT_WARP), as_float_bits(frame), as_float_bits(scene), as_float_bits(xf)};
      F.mats[3 * k + 1] = F4{as_float_bits(first), as_float_bits((uint32_t)m.wlights.size()), 0, 0};
    }
    return any;
  }
  int mat_nest(int m, int guard) const {
    if (guard > 64) throw scene_error("material graph is cyclic");
    const Mat& M = G.mats[m];
    if (M.kind == MAT_LAYERS) { int d = 0; for (int k : M.kids) d = std::max(d, mat_nest(k, guard + 1)); return d + 1; }
    if (M.kind == MAT_BLEND) return 1 + std::max(mat_nest(M.a, guard + 1), mat_nest(M.b, guard + 1));
    return 0;
  }
  int mat_nest_max() const { int d = 0; for (size_t m = 0; m < G.mats.size(); m++) d = std::max(d, mat_nest((int)m, 0)); return d; }

  // composite nesting depth (Tex / Tag / NoShadow / OnlyShadow wrappers are free: the interpreter loops over them); reported
  // in glome_scene_info.  Nothing on the device is unrolled by it any more: all four class methods run over explicit frames
  // (rt_generic.hpp), and what bounds the nesting is the frame memory (vm_words_of below).
  mutable std::unordered_map<int, int> depth_memo;
  int depth_of(int id) const {
    auto it = depth_memo.find(id);
    if (it != depth_memo.end()) return it->second;
    const Node& n = G.at(id);
    int d = 0;
    switch (n.kind) {
      case K_LIST: case K_ISECT: { for (int k : n.kids) d = std::max(d, depth_of(k)); d++; break; }
      case K_INSTANCE: d = depth_of(n.a) + 1; break;
      case K_DIFF: case K_BOUND: case K_INNERBOUND: d = std::max(depth_of(n.a), depth_of(n.b)) + 1; break;
      case K_BIH: { for (auto& bn : n.bih->nodes) for (int k : bn.items) d = std::max(d, depth_of(k)); d++; break; }
      case K_MESH: d = 1; break;
      case K_TEX: case K_TAG: case K_NOSHADOW: case K_ONLYSHADOW: d = depth_of(n.a); break;
      default: break;
    }
    depth_memo[id] = d;
    return d;
  }
  // Frame words a rayint / shadow / inside call on `id` can have live at once in the generic tier's loop (rt_generic.hpp's
  // frame layouts): what the interpreter's nesting limit is now -- memory, checked here so that a scene is refused at commit
  // rather than stopped in the middle of a frame.  An Intersection's chain of frames has two parts (rt_generic.hpp VT_ISECT_HS): a frame
  // for the rest of the list behind a child the ray starts inside of and leaves -- at most one per child but the last, with no advance
  // at all, so commit counts the children --, and a frame per ray advance, which depends on the geometry: the estimate allows
  // kVmIsectChain of those and the run-time check (GLOME_E_LIMIT) remains behind it.
  mutable std::unordered_map<int, int> words_memo, iwords_memo, mwords_memo;
  int warp_words = 0;  // the largest estimate of a Warp material's roots (bind_warps)
  // a Difference of two primitives, an Intersection of primitives that csg_isect's frames hold (emit: RF_PRIMLIST): answered in place,
  // no frame but the word of a shadow call's VT_S_OF_R -- and what `inside` of the node itself takes, should it be a root
  bool csg_in_place(int id) const { auto it = memo.find(id); return it != memo.end() && (it->second.x & RF_PRIMLIST) != 0; }
  int bih_items_max(const Node& n, bool inside) const {
    int d = 0;
    for (auto& bn : n.bih->nodes) for (int k : bn.items) d = std::max(d, inside ? inside_words_of(k) : vm_words_of(k));
    return d;
  }
  int inside_words_of(int id) const {
    auto it = iwords_memo.find(id);
    if (it != iwords_memo.end()) return it->second;
    const Node& n = G.at(id);
    int d = 0;
    switch (n.kind) {
      case K_LIST: case K_ISECT: { for (int k : n.kids) d = std::max(d, inside_words_of(k)); d += 3; break; }
      case K_INSTANCE: d = 4 + inside_words_of(n.a); break;
      case K_DIFF: case K_BOUND: case K_INNERBOUND: d = 3 + std::max(inside_words_of(n.a), inside_words_of(n.b)); break;
      case K_BIH: d = 3 + n.bih->depth + 3 + bih_items_max(n, true); break;
      case K_TEX: case K_TAG: case K_NOSHADOW: case K_ONLYSHADOW: d = inside_words_of(n.a); break;
      default: break;
    }
    iwords_memo[id] = d;
    return d;
  }
  int meta_words_of(int id) const {  // get_metainfo's frames (vm_meta), with the inside calls it makes above them
    auto it = mwords_memo.find(id);
    if (it != mwords_memo.end()) return it->second;
    const Node& n = G.at(id);
    int d = 0;
    switch (n.kind) {
      case K_LIST: case K_ISECT: { for (int k : n.kids) d = std::max(d, std::max(meta_words_of(k), 1 + inside_words_of(k))); d = std::max(d, 1 + inside_words_of(id)) + 7; break; }
      case K_INSTANCE: d = 8 + meta_words_of(n.a); break;
      case K_DIFF: case K_BOUND: case K_INNERBOUND: d = 3 + std::max(std::max(meta_words_of(n.a), meta_words_of(n.b)), 1 + std::max(inside_words_of(n.a), inside_words_of(n.b))); break;
      case K_BIH: { for (auto& bn : n.bih->nodes) for (int k : bn.items) d = std::max(d, std::max(meta_words_of(k), 1 + inside_words_of(k))); d += 11 + n.bih->depth; break; }
      case K_TEX: case K_TAG: case K_NOSHADOW: case K_ONLYSHADOW: d = meta_words_of(n.a); break;
      default: break;
    }
    mwords_memo[id] = d;
    return d;
  }
  int vm_words_of(int id) const {
    auto it = words_memo.find(id);
    if (it != words_memo.end()) return it->second;
    const Node& n = G.at(id);
    int d = 0;
    switch (n.kind) {
      case K_LIST: { for (int k : n.kids) d = std::max(d, vm_words_of(k)); d += kVmListR; break; }
      case K_ISECT: { if (csg_in_place(id)) { d = 1 + inside_words_of(id); break; } for (int k : n.kids) d = std::max(d, std::max(vm_words_of(k), 1 + inside_words_of(k))); d += 1 + ((int)n.kids.size() + kVmIsectChain) * kVmIsectWords; break; }
      case K_INSTANCE: d = kVmInstR + vm_words_of(n.a); break;
      case K_DIFF: if (csg_in_place(id)) { d = 1 + inside_words_of(id); break; } d = 1 + kVmDiffFixed + kCsgMaxAdvance + std::max(std::max(vm_words_of(n.a), vm_words_of(n.b)), 1 + std::max(std::max(inside_words_of(n.a), inside_words_of(n.b)), meta_words_of(n.a))); break;
      case K_BOUND: d = kVmBoundR + std::max(std::max(vm_words_of(n.a), vm_words_of(n.b)), 1 + inside_words_of(n.a)); break;
      case K_INNERBOUND: d = kVmIbR + std::max(vm_words_of(n.a), vm_words_of(n.b)); break;
      case K_BIH: d = kVmBihFixedR + 3 * n.bih->depth + bih_items_max(n, false); break;
      case K_TEX: case K_TAG: case K_NOSHADOW: case K_ONLYSHADOW: d = vm_words_of(n.a); break;
      default: break;  // primitives and a Mesh (its walk has a stack of its own) need no frame
    }
    words_memo[id] = d;
    return d;
  }

  // longest texture stack a hit can carry: the Tex wrappers on a path from `id` down to a primitive (a Mesh adds its
  // per-triangle texture, Mesh.hs:148-150).  The device stack holds kMaxTexDepth materials; a deeper one is refused at
  // commit -- the traversal would silently drop the outermost textures.
  int tex_cap = kMaxTexDepth;  // ids a TexStack holds in this scene
  mutable std::unordered_map<int, int> tex_memo;
  int tex_depth_of(int id) const {
    auto it = tex_memo.find(id);
    if (it != tex_memo.end()) return it->second;
    const Node& n = G.at(id);
    int d = 0;
    switch (n.kind) {
      case K_LIST: case K_ISECT: for (int k : n.kids) d = std::max(d, tex_depth_of(k)); break;
      case K_INSTANCE: case K_TAG: case K_NOSHADOW: case K_ONLYSHADOW: d = tex_depth_of(n.a); break;
      case K_DIFF: case K_BOUND: case K_INNERBOUND: d = std::max(tex_depth_of(n.a), tex_depth_of(n.b)); break;
      case K_BIH: for (auto& bn : n.bih->nodes) for (int k : bn.items) d = std::max(d, tex_depth_of(k)); break;
      case K_MESH: for (const MeshTri& t : n.mesh->tris) if (t.tex >= 0) { d = 1; break; } break;
      case K_TEX: d = tex_depth_of(n.a) + 1; break;
      default: break;
    }
    tex_memo[id] = d;
    return d;
  }

  // Which emitted meshes may have their vertices replaced in the committed scene (MeshUpdateInfo::plain): every one that no Bih
  // lies above, on any path from the root or from a Warp material's frame / scene.  Of the composites, only a Bih keeps something derived
  // from a child's bound -- its planes and its root box.  A list, an Instance, a Difference, an Intersection and the Tex / Tag / shadow
  // wrappers emit no box at all (emit, below), and the bounding solid of a Bound / InnerBound is the caller's own object.
  // And which triangle bihs may have their triangles replaced (LeafBihUpdateInfo::plain): every one that no OTHER Bih lies above -- for
  // the same reason -- and whose item triangles the scene reaches through this bih alone: a triangle node that is also in a group beside
  // the bih, or in another bih, has a record of its own there, which an update of this bih could not move.
  // And which Instances may have their matrices replaced (InstanceUpdateInfo::plain).  An Instance's matrix is read from its xfm
  // slots alone, so one with no Bih above it on any path is a write of those slots.  One that IS an item of a bih (wrappers only in
  // between), that bih having no other above it, also moves the item's box: that tree's planes and box are refitted from the tables of
  // emit_bih.  Refused: an Instance that lies deeper inside an item (the item's box depends on it through a list, a CSG node, a Bound or
  // another Instance, which the update does not recompute), one with two or more bihs above it on some path (the outer tree's item box is
  // the inner tree's box), and one that is an item more than once (a single table entry could not name both).
  // And which sphere bihs may have their spheres replaced: exactly as a triangle bih, Sphere for Triangle -- one record, one rule.
  void mark_updatable(int root) {
    if (F.mesh_updates.empty() && F.leaf_bih_updates.empty() && F.inst_updates.empty()) return;
    std::unordered_map<int, size_t> slot_of, bslot_of, islot_of;
    for (size_t k = 0; k < F.mesh_updates.size(); k++) slot_of[F.mesh_updates[k].node] = k;
    for (size_t k = 0; k < F.leaf_bih_updates.size(); k++) bslot_of[F.leaf_bih_updates[k].node] = k;
    for (size_t k = 0; k < F.inst_updates.size(); k++) islot_of[F.inst_updates[k].node] = k;
    for (const InstItem& I : inst_items) {
      InstanceUpdateInfo& U = F.inst_updates[islot_of.at(I.inst)];
      if (U.bih >= 0 && U.plain.ok) {
        U.plain.ok = false;
        U.plain.why_not = "instance " + std::to_string(I.inst) + " is an item of a bih more than once (bih " + std::to_string(U.bih) + " and bih " + std::to_string(I.bih) + ")";
      }
      U.bih = I.bih; U.item = I.item;
    }
    // per Triangle and Sphere node, the innermost Bih it was reached under: kUnseen, a bih's id, -1 for none, kMixed once two of those differ
    constexpr int kUnseen = -3, kMixed = -2;
    std::vector<int> tri_under(F.leaf_bih_updates.empty() ? 0 : G.nodes.size(), kUnseen);
    struct Item { int id, bih, inner, direct; };  // bih: the outermost Bih above, inner: the innermost (-1: none), direct: only wrappers since that bih's item list
    struct Seen { int bih, inner, direct; bool operator==(const Seen& o) const { return bih == o.bih && inner == o.inner && direct == o.direct; } };
    std::unordered_map<int, std::vector<Seen>> seen;  // composites and wrappers only (a primitive has nothing below it): the states a node was visited with
    std::vector<Item> stack{{root, -1, -1, 0}};
    for (const Mat& m : G.mats) if (m.kind == MAT_WARP) { stack.push_back({m.wframe, -1, -1, 0}); if (m.wscene >= 0) stack.push_back({m.wscene, -1, -1, 0}); }
    while (!stack.empty()) {
      Item it = stack.back();
      stack.pop_back();
      const Node& n = G.at(it.id);
      if (is_prim(n.kind) || n.kind == K_VOID) {
        if ((n.kind == K_TRI || n.kind == K_SPHERE) && !tri_under.empty()) { int& u = tri_under[(size_t)it.id]; u = (u == kUnseen || u == it.inner) ? it.inner : kMixed; }
        continue;
      }
      std::vector<Seen>& sn = seen[it.id];
      if (std::find(sn.begin(), sn.end(), Seen{it.bih, it.inner, it.direct}) != sn.end()) continue;
      sn.push_back({it.bih, it.inner, it.direct});
      switch (n.kind) {
        case K_LIST: case K_ISECT: for (int k : n.kids) stack.push_back({k, it.bih, it.inner, 0}); break;
        case K_DIFF: case K_BOUND: case K_INNERBOUND: stack.push_back({n.a, it.bih, it.inner, 0}); stack.push_back({n.b, it.bih, it.inner, 0}); break;
        case K_INSTANCE: {
          auto sl = islot_of.find(it.id);
          if (sl != islot_of.end() && F.inst_updates[sl->second].plain.ok && it.bih >= 0) {
            InstanceUpdateInfo& U = F.inst_updates[sl->second];
            if (it.bih != it.inner) {
              U.plain.ok = false;
              U.plain.why_not = "instance " + std::to_string(it.id) + " lies under bih " + std::to_string(it.inner) + " inside bih " + std::to_string(it.bih) + ", whose planes and root box were built from the inner tree's bound";
            } else if (!it.direct) {
              U.plain.ok = false;
              U.plain.why_not = "instance " + std::to_string(it.id) + " lies inside an item of bih " + std::to_string(it.inner) + " rather than being the item: that item's box depends on it through a list, CSG, Bound or Instance, which an update does not recompute";
            }
          }
          stack.push_back({n.a, it.bih, it.inner, 0});
          break;
        }
        case K_TEX: case K_TAG: case K_NOSHADOW: case K_ONLYSHADOW: stack.push_back({n.a, it.bih, it.inner, it.direct}); break;
        case K_BIH: {
          auto sl = bslot_of.find(it.id);
          if (it.bih >= 0 && sl != bslot_of.end() && F.leaf_bih_updates[sl->second].plain.ok) {
            LeafBihUpdateInfo& U = F.leaf_bih_updates[sl->second];
            U.plain.ok = false;
            U.plain.why_not = "bih " + std::to_string(it.id) + " lies inside bih " + std::to_string(it.bih) + ", whose planes and root box were built from its bound";
          }
          for (auto& bn : n.bih->nodes) for (int k : bn.items) stack.push_back({k, it.bih < 0 ? it.id : it.bih, it.id, 1});
          break;
        }
        case K_MESH: {
          auto sl = slot_of.find(it.id);
          if (it.bih >= 0 && sl != slot_of.end() && F.mesh_updates[sl->second].plain.ok) {
            MeshUpdateInfo& U = F.mesh_updates[sl->second];
            U.plain.ok = false;
            U.plain.why_not = "mesh " + std::to_string(it.id) + " lies inside bih " + std::to_string(it.bih) + ", whose planes and root box were built from the mesh's bound";
          }
          break;
        }
        default: break;
      }
    }
    for (LeafBihUpdateInfo& U : F.leaf_bih_updates) {
      if (!U.plain.ok) continue;
      const std::string why = item_outside(U, tri_under);
      if (!why.empty()) { U.plain.ok = false; U.plain.why_not = why; }
    }
  }
  // A leaf bih's item that the scene also reaches outside that bih (tri_under: mark_updatable), named; empty: none.  BC_TRI and BC_SPHERE
  // items are emitted fresh, so such a copy has a second record, which an update of this bih could not move.
  std::string item_outside(const LeafBihUpdateInfo& U, const std::vector<int>& under) const {
    constexpr int kUnseen = -3;
    for (const BihTree::Node& bn : G.at(U.node).bih->nodes)
      for (int item : bn.items) {
        const int t = G.peel_wrappers(item);
        const int u = under[(size_t)t];
        if (u == U.node || u == kUnseen) continue;  // (kUnseen: the bih itself is not reachable from the root -- nothing renders it)
        return std::string(U.item_word()) + " " + std::to_string(t) + " of bih " + std::to_string(U.node) + " is also part of the scene outside that bih, as a copy an update could not move";
      }
    return std::string();
  }

  // The second answer (NestedAnswer), for glome_scene_nested_updates: an update of X -- a Mesh, a triangle bih, an Instance that is an
  // item of a bih -- is accepted when every bih above it can be refitted from the tables of emit_bih, one tree after the other.  An item
  // of a bih B is LIVE OVER Z when peeling its wrappers gives Z (a direct item) or an Instance whose child, peeled again, is Z (an
  // instanced item).  X is ok when on every path from a root to X each bih B on the path holds, on that path, an item that is live over
  // the next thing down the path: X, or the next bih.  (For an Instance X its own bih holds X as the item.)  Anything else between two
  // trees -- a list, a CSG node, a Bound / InnerBound, a second Instance -- is refused with the node in the way named: its box is
  // derived from the object's by something no kernel makes again.  One object under several items or several bihs is fine: every one
  // of those rows is derived from the same bound.  The walk records, per Mesh, Bih and Instance, the states it was reached in
  // (innermost bih, what lies between that bih's item list and the node); the answers are then resolved bih by bih, memoised.
  void mark_nested(int root) {
    if (F.mesh_updates.empty() && F.leaf_bih_updates.empty() && F.inst_updates.empty() && F.inst_bihs.empty()) return;
    enum { kDirect = 0, kInst = 1, kBroken = 2 };
    struct Edge { int bih, link, blocker, via; };   // blocker: the first list / CSG / Bound / second Instance since the item list; via: the Instance passed first (-1: none)
    struct Item { int id, inner, link, blocker, via; };
    constexpr int kUnseen = -3, kMixed = -2;
    std::vector<int> tri_under(F.leaf_bih_updates.empty() ? 0 : G.nodes.size(), kUnseen);
    std::unordered_map<int, std::vector<Edge>> edges;
    std::unordered_map<int, std::vector<std::pair<int, int>>> seen;
    std::vector<Item> stack{{root, -1, kDirect, -1, -1}};
    for (const Mat& m : G.mats) if (m.kind == MAT_WARP) { stack.push_back({m.wframe, -1, kDirect, -1, -1}); if (m.wscene >= 0) stack.push_back({m.wscene, -1, kDirect, -1, -1}); }
    while (!stack.empty()) {
      const Item it = stack.back();
      stack.pop_back();
      const Node& n = G.at(it.id);
      if (is_prim(n.kind) || n.kind == K_VOID) {
        if ((n.kind == K_TRI || n.kind == K_SPHERE) && !tri_under.empty()) { int& u = tri_under[(size_t)it.id]; u = (u == kUnseen || u == it.inner) ? it.inner : kMixed; }
        continue;
      }
      std::vector<std::pair<int, int>>& sn = seen[it.id];
      if (std::find(sn.begin(), sn.end(), std::make_pair(it.inner, it.link)) != sn.end()) continue;
      sn.push_back({it.inner, it.link});
      // below a node that is no wrapper: nothing is live any more (no bih above: nothing to keep track of)
      const Item below{0, it.inner, it.inner < 0 ? kDirect : kBroken, it.inner < 0 ? -1 : (it.link == kBroken ? it.blocker : it.id), it.via};  // (the first node in the way is the one named)
      switch (n.kind) {
        case K_LIST: case K_ISECT: for (int k : n.kids) stack.push_back({k, below.inner, below.link, below.blocker, below.via}); break;
        case K_DIFF: case K_BOUND: case K_INNERBOUND: stack.push_back({n.a, below.inner, below.link, below.blocker, below.via}); stack.push_back({n.b, below.inner, below.link, below.blocker, below.via}); break;
        case K_INSTANCE:
          edges[it.id].push_back({it.inner, it.link, it.blocker, it.via});
          if (it.inner >= 0 && it.link == kDirect) stack.push_back({n.a, it.inner, kInst, -1, it.id});
          else stack.push_back({n.a, below.inner, below.link, below.blocker, below.via});
          break;
        case K_TEX: case K_TAG: case K_NOSHADOW: case K_ONLYSHADOW: stack.push_back({n.a, it.inner, it.link, it.blocker, it.via}); break;
        case K_BIH:
          edges[it.id].push_back({it.inner, it.link, it.blocker, it.via});
          for (auto& bn : n.bih->nodes) for (int k : bn.items) stack.push_back({k, it.id, kDirect, -1, -1});
          break;
        case K_MESH: edges[it.id].push_back({it.inner, it.link, it.blocker, it.via}); break;
        default: break;
      }
    }
    // a tree's height among the trees: the longest chain of bihs below it (what orders `above`)
    std::unordered_map<int, std::vector<int>> kids_of;
    for (auto& e : edges) if (G.at(e.first).kind == K_BIH) for (const Edge& ed : e.second) if (ed.bih >= 0) kids_of[ed.bih].push_back(e.first);
    std::unordered_map<int, int> height_memo;
    std::function<int(int)> height = [&](int b) {
      auto f = height_memo.find(b);
      if (f != height_memo.end()) return f->second;
      int h = 0;
      for (int c : kids_of[b]) h = std::max(h, height(c) + 1);
      return height_memo[b] = h;
    };
    auto what = [&](int id) { const int k = G.at(id).kind; return std::string(k == K_MESH ? "mesh " : (k == K_BIH ? "bih " : "instance ")) + std::to_string(id); };
    std::unordered_map<int, NestedAnswer> bih_memo;
    std::function<NestedAnswer(int)> answer = [&](int x) {
      const bool is_bih = G.at(x).kind == K_BIH, is_inst = G.at(x).kind == K_INSTANCE;
      if (is_bih) { auto f = bih_memo.find(x); if (f != bih_memo.end()) return f->second; }
      NestedAnswer A;
      std::set<int> above;
      auto f = edges.find(x);
      if (f != edges.end()) for (const Edge& e : f->second) {
        if (e.bih < 0) continue;
        if (e.link == kBroken || (is_inst && e.link == kInst)) {
          A.ok = false;
          // for an Instance the first thing in the way is an Instance above it (it is then not the item); for a Mesh or Bih one Instance is fine
          const int in_the_way = (is_inst && e.via >= 0) ? e.via : e.blocker;
          A.why_not = what(x) + " lies inside an item of bih " + std::to_string(e.bih) + " under " + kind_name(G.at(in_the_way).kind) + " " + std::to_string(in_the_way) +
                      ": that item's box depends on it through a list, CSG, Bound or second Instance, which a refit does not recompute";
          break;
        }
        const NestedAnswer up = answer(e.bih);
        if (!up.ok) { A.ok = false; A.why_not = up.why_not; break; }
        above.insert(e.bih);
        above.insert(up.above.begin(), up.above.end());
      }
      if (A.ok) {
        A.above.assign(above.begin(), above.end());
        std::stable_sort(A.above.begin(), A.above.end(), [&](int a, int b) { return height(a) < height(b); });
      }
      if (is_bih) bih_memo[x] = A;
      return A;
    };
    for (MeshUpdateInfo& U : F.mesh_updates) U.nested = answer(U.node);
    for (LeafBihUpdateInfo& U : F.leaf_bih_updates) {
      if (U.plain.why_not.rfind("bih " + std::to_string(U.node) + " holds " + U.item_word(), 0) == 0) { U.nested.ok = false; U.nested.why_not = U.plain.why_not; continue; }  // (emit_bih's refusal)
      U.nested = answer(U.node);
      if (!U.nested.ok) continue;
      const std::string why = item_outside(U, tri_under);
      if (!why.empty()) { U.nested.ok = false; U.nested.why_not = why; }
    }
    std::unordered_map<int, std::pair<int, int>> item_of_bih;  // Instance -> (its first bih, how often it is an item)
    for (const InstItem& I : inst_items) { auto r = item_of_bih.insert({I.inst, {I.bih, 0}}); r.first->second.second++; }
    for (InstanceUpdateInfo& U : F.inst_updates) {
      auto f = item_of_bih.find(U.node);
      if (f != item_of_bih.end() && f->second.second > 1) {
        U.nested.ok = false;
        U.nested.why_not = "instance " + std::to_string(U.node) + " is an item of a bih more than once (bih " + std::to_string(f->second.first) + " and bih " + std::to_string(U.bih) + ")";
        continue;
      }
      U.nested = answer(U.node);
    }
    for (InstBihInfo& B : F.inst_bihs) B.nested = answer(B.node);
  }

  // ---- primitive pools ----
  uint32_t emit_tri(const double* p) {  // (p1, e1, e2, n) evaluated in double, rounded once
    D3 p1{p[0], p[1], p[2]}, p2{p[3], p[4], p[5]}, p3{p[6], p[7], p[8]};
    D3 e1 = p2 - p1, e2 = p3 - p1;
    D3 n = normalize(cross(e1, e2));  // vnorm $ vcross e1 e2, Triangle.hs:73
    uint32_t idx = (uint32_t)(F.tris.size() / 3);
    F.tris.push_back(mk4(p1.x, p1.y, p1.z, n.x));
    F.tris.push_back(mk4(e1.x, e1.y, e1.z, n.y));
    F.tris.push_back(mk4(e2.x, e2.y, e2.z, n.z));
    return idx;
  }
  U4 emit_prim(const Node& n) {
    const double* p = n.p;
    U4 r{0, 0, 0, (uint32_t)n.uid};
    switch (n.kind) {
      case K_SPHERE: r.x = R_SPHERE; r.y = (uint32_t)F.spheres.size(); F.spheres.push_back(mk4(p[0], p[1], p[2], p[3])); break;
      case K_TRI: r.x = R_TRI; r.y = emit_tri(p); break;
      case K_TRIN: {  // self-contained 6-word block in the trinorms heap
        D3 p1{p[0], p[1], p[2]}, p2{p[3], p[4], p[5]}, p3{p[6], p[7], p[8]};
        D3 e1 = p2 - p1, e2 = p3 - p1;
        r.x = R_TRIN; r.y = (uint32_t)F.trinorms.size();
        F.trinorms.push_back(mk4(p1.x, p1.y, p1.z, 0)); F.trinorms.push_back(mk4(e1.x, e1.y, e1.z, 0)); F.trinorms.push_back(mk4(e2.x, e2.y, e2.z, 0));
        for (int k = 0; k < 3; k++) F.trinorms.push_back(mk4(p[9 + 3 * k], p[10 + 3 * k], p[11 + 3 * k], 0));
        F.n_other_prims++;
        break;
      }
      case K_BOX: r.x = R_BOX; r.y = (uint32_t)(F.boxes.size() / 2); F.boxes.push_back(mk4(p[0], p[1], p[2], 0)); F.boxes.push_back(mk4(p[3], p[4], p[5], 0)); F.n_other_prims++; break;
      case K_PLANE: r.x = R_PLANE; r.y = (uint32_t)F.planes.size(); F.planes.push_back(mk4(p[0], p[1], p[2], p[3])); F.n_other_prims++; break;
      case K_DISC: r.x = R_DISC; r.y = (uint32_t)(F.discs.size() / 2); F.discs.push_back(mk4(p[0], p[1], p[2], p[6])); F.discs.push_back(mk4(p[3], p[4], p[5], 0)); F.n_other_prims++; break;
      case K_CYL: r.x = R_CYL; r.y = (uint32_t)F.quadrics.size(); F.quadrics.push_back(mk4(p[0], p[1], p[2], 0)); F.n_other_prims++; break;
      case K_CONE: r.x = R_CONE; r.y = (uint32_t)F.quadrics.size(); F.quadrics.push_back(mk4(p[0], p[1], p[2], p[3])); F.n_other_prims++; break;
      default: break;
    }
    return r;
  }

  // Peel Tex / Tag / NoShadow / OnlyShadow wrappers off a node.  Up to two Tex levels fold into a primitive's
  // own stack (innermost first, id+1, 16 bits each); flags fold into the record.
  struct Peeled { int id; uint32_t flags; uint32_t own; int ntex; };
  Peeled peel(int id) const {
    Peeled p{id, 0, 0, 0};
    std::vector<int> texs;  // outermost first
    for (;;) {
      const Node& n = G.at(p.id);
      if (n.kind == K_TEX) { texs.push_back(n.mat); p.id = n.a; }
      else if (n.kind == K_TAG) p.id = n.a;
      else if (n.kind == K_NOSHADOW) { p.flags |= RF_NOSHADOW; p.id = n.a; }
      else if (n.kind == K_ONLYSHADOW) { p.flags |= RF_NOVIS; p.id = n.a; }
      else break;
    }
    p.ntex = (int)texs.size();
    // head of the stack = innermost Tex = last in `texs`
    if (p.ntex <= 2) for (int k = 0; k < p.ntex; k++) p.own |= (uint32_t)(texs[p.ntex - 1 - k] + 1) << (16 * k);
    return p;
  }

  // "CSG over primitives": what the flat tier evaluates without recursion (rt_device.hpp csg_item_rayint) -- a primitive, a
  // Difference or Intersection whose operands are primitives, or an Instance of one of those (how `cylinder` / `cone` and
  // TestScene.hs's transformed CSG shapes arrive); Tex / Tag / shadow-flag wrappers anywhere in between.
  bool prim_under_wrappers(int id) const { return is_prim(G.at(peel(id).id).kind); }
  bool csg_core(int id) const {
    const Node& c = G.at(peel(id).id);
    if (c.kind == K_DIFF) return prim_under_wrappers(c.a) && prim_under_wrappers(c.b);
    if (c.kind == K_ISECT) {
      // (csg_isect's frames: one per list position it may nest through, and a few for advances before they fold in place; a longer
      // Intersection is the generic tier's, whose frames are sized per scene)
      if ((int)c.kids.size() + 8 > kIsectFrames) return false;
      for (int k : c.kids) if (!prim_under_wrappers(k)) return false;
      return true;
    }
    return false;
  }
  bool csg_simple(int id) const {
    const Node& c = G.at(peel(id).id);
    if (is_prim(c.kind)) return true;
    if (c.kind == K_INSTANCE) return prim_under_wrappers(c.a) || csg_core(c.a);
    return csg_core(id);
  }

  // emit(id) -> the record VALUE for a reference to node id (children are written into F.recs / pools)
  U4 emit(int id) {
    auto it = memo.find(id);
    if (it != memo.end()) return it->second;
    const Node& n = G.at(id);
    U4 r{R_VOID, 0, 0, (uint32_t)n.uid};
    switch (n.kind) {
      case K_VOID: break;
      case K_SPHERE: case K_TRI: case K_TRIN: case K_BOX: case K_PLANE: case K_DISC: case K_CYL: case K_CONE: r = emit_prim(n); break;
      case K_TEX: case K_TAG: case K_NOSHADOW: case K_ONLYSHADOW: {
        Peeled p = peel(id);
        const Node& c = G.at(p.id);
        if (is_prim(c.kind) && p.ntex <= 2) {  // fold into the primitive's record
          r = emit(p.id);
          r.x |= p.flags; r.z = p.own;
        } else if (n.kind == K_TEX) {  // explicit Tex record over the child
          U4 child = emit(n.a);
          r.x = R_TEX; r.y = slot(child); r.z = (uint32_t)n.mat;
        } else {  // Tag / NoShadow / OnlyShadow over a composite: flags on a copy of the child's record
          r = emit(n.a);
          if (n.kind == K_NOSHADOW) r.x |= RF_NOSHADOW;
          if (n.kind == K_ONLYSHADOW) r.x |= RF_NOVIS;
        }
        break;
      }
      case K_LIST: case K_ISECT: {
        std::vector<U4> kids;
        for (int k : n.kids) kids.push_back(emit(k));
        r.x = (n.kind == K_LIST) ? R_LIST : R_ISECT;
        if (!kids.empty()) {  // (a list or an Intersection of primitives: the generic tier answers those in place)
          bool prims = true;
          for (const U4& kr : kids) { const uint32_t kk = kr.x & RF_KINDMASK; prims = prims && kk >= R_SPHERE && kk <= R_CONE; }
          if (prims && (n.kind == K_LIST || (int)kids.size() + 8 <= kIsectFrames)) r.x |= RF_PRIMLIST;  // (csg_isect's frames: see csg_core)
        }
        r.y = (uint32_t)F.recs.size(); r.z = (uint32_t)kids.size();
        F.recs.insert(F.recs.end(), kids.begin(), kids.end());
        break;
      }
      case K_INSTANCE: {
        U4 child = emit(n.a);
        r.x = R_INSTANCE; r.y = slot(child); r.z = (uint32_t)(F.xfms.size() / 6);
        for (int k = 0; k < 3; k++) F.xfms.push_back(mk4(n.xf.f.m[4 * k], n.xf.f.m[4 * k + 1], n.xf.f.m[4 * k + 2], n.xf.f.m[4 * k + 3]));
        for (int k = 0; k < 3; k++) F.xfms.push_back(mk4(n.xf.i.m[4 * k], n.xf.i.m[4 * k + 1], n.xf.i.m[4 * k + 2], n.xf.i.m[4 * k + 3]));
        InstanceUpdateInfo U;
        U.node = id; U.slots.push_back(r.z);
        F.inst_updates.push_back(std::move(U));
        break;
      }
      case K_DIFF: case K_BOUND: case K_INNERBOUND: {
        U4 a = emit(n.a), b = emit(n.b);
        r.x = n.kind == K_DIFF ? R_DIFF : (n.kind == K_BOUND ? R_BOUND : R_INNERBOUND);
        if (n.kind == K_DIFF) {  // (a Difference of two primitives: answered in place by the generic tier)
          const uint32_t ka = a.x & RF_KINDMASK, kb = b.x & RF_KINDMASK;
          if (ka >= R_SPHERE && ka <= R_CONE && kb >= R_SPHERE && kb <= R_CONE) r.x |= RF_PRIMLIST;
          if (n.retex) r.x |= RF_RETEX;
        }
        r.y = slot(a); r.z = slot(b);
        break;
      }
      case K_BIH: r = emit_bih(n, id); break;
      case K_MESH: r = emit_mesh(n, id); break;
    }
    memo[id] = r;
    return r;
  }
  uint32_t slot(const U4& v) { F.recs.push_back(v); return (uint32_t)F.recs.size() - 1; }

  // An item the interpreter answers in place whatever the ray (rt_generic.hpp: vm_resolve_r / _s return 0 or 1, or vm_inst_prim_hit /
  // vm_inst_prim_shadow take it): a primitive, or an Instance of a primitive or of a list of primitives, under Tex wrappers on either
  // side.  A BIH made of such items alone is walked as a packet by the interpreter's service (bih_items_wave).
  bool item_in_place(U4 c) const {
    while ((c.x & RF_KINDMASK) == R_TEX) c = F.recs[c.y];
    uint32_t k = c.x & RF_KINDMASK;
    if (k >= R_SPHERE && k <= R_CONE) return true;
    if (k != R_INSTANCE) return false;
    c = F.recs[c.y];
    while ((c.x & RF_KINDMASK) == R_TEX) c = F.recs[c.y];
    k = c.x & RF_KINDMASK;
    return (k >= R_SPHERE && k <= R_CONE) || (k == R_LIST && (c.x & RF_PRIMLIST) != 0);
  }

  // A branch's two planes as the device holds them.  A child that is an empty leaf (a quarter of the leaves the reference builder makes)
  // gets a plane at -inf / +inf: the interval tests of the traversal (`near < t1`, `t2 < far`) then fail for it whatever the ray, so
  // the device never enters it and needs no test for it.  The other child's interval does not depend on this plane.
  static void branch_planes(const BihTree::Node& bn, const std::vector<uint32_t>& ref, float& ls, float& rs) {
    const float inf = std::numeric_limits<float>::infinity();
    ls = ref[(size_t)bn.left] == BREF_LEAF_BIT ? -inf : round_up(bn.lsplit);
    rs = ref[(size_t)bn.right] == BREF_LEAF_BIT ? inf : round_down(bn.rsplit);
  }

  // A triangle or sphere bih (emit_bih, which has reserved the header and the node slots): where everything goes is leaf_bih_layout's,
  // which reads no coordinate; the values -- records, pool entries, pair values, planes, the box -- are filled in here.
  U4 emit_leaf_bih(const Node& n, int id, uint32_t cls, uint32_t hdr, uint32_t base) {
    const BihTree& T = *n.bih;
    LeafBihUpdateInfo U;  // its update tables
    U.node = id; U.cls = cls; U.row_words = cls == BC_TRI ? 2u : 1u; U.hdr = hdr; U.first_slot = base;
    const std::vector<int> order = T.update_order();
    U.n_items = (int)order.size();
    std::vector<uint32_t> item_of(G.nodes.size(), 0xffffffffu);  // item node id -> its index in the update order (whichever way the tree was made)
    std::vector<char> prim_seen(G.nodes.size(), 0);  // an item, or a primitive under two items, that the tree holds twice has two records: one row cannot name both
    for (size_t k = 0; k < order.size(); k++) {
      const int t = G.peel_wrappers(order[k]);
      if ((item_of[(size_t)order[k]] != 0xffffffffu || prim_seen[(size_t)t]) && U.plain.ok) {
        U.plain.ok = false;
        U.plain.why_not = "bih " + std::to_string(id) + " holds " + U.item_word() + " " + std::to_string(t) + " more than once";
      }
      item_of[(size_t)order[k]] = (uint32_t)k; prim_seen[(size_t)t] = 1;
    }
    const uint32_t first_rec = (uint32_t)F.recs.size(), first_prim = (uint32_t)(cls == BC_TRI ? F.tris.size() / 3 : F.spheres.size());
    LeafBihLayout L = leaf_bih_layout(T, cls, item_of, base, first_rec, first_prim, (uint64_t)F.tripairs.size());
    size_t pair_rec = 0;
    for (size_t k = 0; k < T.nodes.size(); k++) {
      const BihTree::Node& bn = T.nodes[k];
      if (!bn.leaf) continue;
      const uint32_t count = (uint32_t)bn.items.size(), at = L.leaf_first[k];
      for (uint32_t q = 0; q < count; q++) {
        Peeled p = peel(bn.items[q]);
        U4 rec = emit_prim(G.at(p.id));
        rec.x |= p.flags; rec.z = p.own;
        if (rec.y != first_prim + at + q) throw scene_error("internal: BIH leaf pools are not contiguous");  // (both are emitted in leaf order)
        F.recs.push_back(rec);
      }
      if (!L.paired[k]) continue;
      if ((emit_pairs(first_prim + at, count, &L.pair_words[2 * pair_rec]) | 3u) != L.pkleaf[k]) throw scene_error("internal: BIH pair records are not contiguous");
      pair_rec += (count + 1u) / 2u;
    }
    for (uint32_t s = 0; s < std::max<uint32_t>(L.n_slots, 1u); s++) F.bihnodes[base + s] = F4{0.0f, 0.0f, as_float_bits(L.node_zw[2 * (size_t)s]), as_float_bits(L.node_zw[2 * (size_t)s + 1])};
    for (size_t k = 0; k < T.nodes.size(); k++) {
      const BihTree::Node& bn = T.nodes[k];
      if (bn.leaf) continue;
      const size_t s = L.slot[k];
      float ls, rs;
      branch_planes(bn, L.ref, ls, rs);
      F.bihnodes[base + s].x = ls; F.bihnodes[base + s].y = rs;
      if (L.pk) F.pknodes[base + s] = F4{ls, rs, as_float_bits(L.pk_zw[2 * s]), as_float_bits(L.pk_zw[2 * s + 1])};
    }
    F.bihhdr[3 * hdr] = mk4u(round_down(T.bb.lo.x), round_down(T.bb.lo.y), round_down(T.bb.lo.z), L.ref[0]);
    F.bihhdr[3 * hdr + 1] = mk4u(round_up(T.bb.hi.x), round_up(T.bb.hi.y), round_up(T.bb.hi.z), cls);
    F.bihhdr[3 * hdr + 2] = F4{as_float_bits(L.hdr2[0]), as_float_bits(L.hdr2[1]), as_float_bits(L.hdr2[2]), as_float_bits(L.hdr2[3])};
    if (cls == BC_TRI) F.pk_all = F.pk_all && L.pk;
    F.max_sphere_bih_depth = std::max(F.max_sphere_bih_depth, T.depth);
    U.n_slots = L.n_slots; U.n_recs = L.n_recs; U.pk = L.pk; U.n_pair_recs = L.n_pair_recs; U.first_pair_word = L.first_pair_word; U.depth = T.depth;
    if (L.n_recs) { U.first_prim = first_prim; U.first_rec = first_rec; }
    U.rows = std::move(L.rows); U.level_nodes = std::move(L.level_nodes); U.level_off = std::move(L.level_off);
    box6(T.bb, U.bound6);
    F.leaf_bih_updates.push_back(std::move(U));
    movable_bihs.insert(id);
    return U4{R_BIH, hdr, 0, (uint32_t)n.uid};
  }

  // BIH: nodes in preorder; leaf items become consecutive records, and (for homogeneous leaves) consecutive pool
  // entries, so a leaf is one contiguous run of 48-byte triangles / 16-byte spheres.
  U4 emit_bih(const Node& n, int id) {
    const BihTree& T = *n.bih;
    F.max_bih_depth = std::max(F.max_bih_depth, T.depth);
    // classify
    bool all_tri = true, all_sph = true, all_simple = true, all_csg = true;
    for (auto& bn : T.nodes) for (int it : bn.items) {
      Peeled p = peel(it);
      const Node& c = G.at(p.id);
      bool simple = is_prim(c.kind) && p.ntex <= 2;
      all_simple &= simple;
      all_tri &= simple && c.kind == K_TRI && p.flags == 0;
      all_sph &= simple && c.kind == K_SPHERE && p.flags == 0;
      all_csg &= csg_simple(it);
    }
    uint32_t cls = all_tri ? BC_TRI : (all_sph ? BC_SPHERE : (all_simple ? BC_SIMPLE : (all_csg ? BC_CSG : BC_GENERIC)));
    uint32_t hdr = (uint32_t)(F.bihhdr.size() / 3);
    F.bihhdr.resize(F.bihhdr.size() + 3);  // reserved now: items of a generic BIH may emit nested BIHs before we fill it
    // Node slots (bih_slots): treelets of branches, then the leaves of 7+ items
    std::vector<uint32_t> slot;
    uint32_t base = (uint32_t)F.bihnodes.size();
    base = (base + 3u) & ~3u;  // line-align this tree's first treelet
    const uint32_t nslots = bih_slots(T, slot);
    F.bihnodes.resize(base + std::max<uint32_t>(nslots, 1u));
    if (base + nslots >= BREF_FIRST_LIMIT) throw limit_error("too many BIH nodes");
    // The primitive classes (BC_TRI, BC_SPHERE, BC_SIMPLE) emit their items fresh, without the memo, so their pool entries are consecutive
    // and leaf follows leaf; the items of BC_CSG / BC_GENERIC go through the memoising emit(): a node shared with another parent keeps one
    // record value (an Instance: one xfm slot), and an item's own records lie between the leaves
    if (cls == BC_TRI || cls == BC_SPHERE) {
      F.pknodes.resize(F.bihnodes.size(), F4{0, 0, 0, 0});
      return emit_leaf_bih(n, id, cls, hdr, base);
    }
    F.pknodes.resize(F.bihnodes.size(), F4{0, 0, 0, 0});
    // pass 1: leaves -- a leaf's item records are consecutive, and so the child reference that describes each leaf is built here
    // (rt_device.hpp: BREF_*)
    std::vector<uint32_t> ref(T.nodes.size(), 0);
    bool in_place = true;
    std::vector<int> item_ids;        // a bih of class BC_CSG / BC_GENERIC: its items in emission order, and their records
    std::vector<uint32_t> item_recs;
    bool has_inst = false;            // ... one of them is an Instance (under wrappers): the tree gets an InstBihInfo
    for (size_t k = 0; k < T.nodes.size(); k++) {
      const BihTree::Node& bn = T.nodes[k];
      if (!bn.leaf) { ref[k] = base + slot[k]; continue; }
      std::vector<U4> items;
      for (size_t q = 0; q < bn.items.size(); q++) {
        int it = bn.items[q];
        U4 rec;
        if (cls == BC_GENERIC || cls == BC_CSG) rec = emit(it);
        else {
          Peeled p = peel(it);
          rec = emit_prim(G.at(p.id));
          rec.x |= p.flags; rec.z = p.own;
        }
        in_place = in_place && item_in_place(rec);
        items.push_back(rec);
      }
      uint32_t first_rec = (uint32_t)F.recs.size();
      F.recs.insert(F.recs.end(), items.begin(), items.end());
      if (cls == BC_GENERIC || cls == BC_CSG) for (size_t q = 0; q < bn.items.size(); q++) {
        item_ids.push_back(bn.items[q]); item_recs.push_back(first_rec + (uint32_t)q);
        int live_obj;
        has_inst = has_inst || item_kind(bn.items[q], live_obj) != InstBihInfo::kStatic;
      }
      if (first_rec + items.size() >= BREF_FIRST_LIMIT) throw limit_error("too many records for the BIH leaf references");
      uint32_t count = (uint32_t)items.size();
      if (count == 0) ref[k] = BREF_LEAF_BIT;
      else if (count <= 6) ref[k] = BREF_LEAF_BIT | (count << 26) | first_rec;
      else {
        F.bihnodes[base + slot[k]] = F4{0.0f, 0.0f, as_float_bits(count), as_float_bits(first_rec)}; ref[k] = BREF_LEAF_BIT | (7u << 26) | (base + slot[k]);
      }
    }
    // pass 2: branches
    for (size_t k = 0; k < T.nodes.size(); k++) {
      const BihTree::Node& bn = T.nodes[k];
      if (bn.leaf) continue;
      float ls, rs;
      branch_planes(bn, ref, ls, rs);
      F.bihnodes[base + slot[k]] = F4{ls, rs, as_float_bits((uint32_t)bn.axis | (ref[bn.left] << 2)), as_float_bits(ref[bn.right])};
    }
    F.bihhdr[3 * hdr] = mk4u(round_down(T.bb.lo.x), round_down(T.bb.lo.y), round_down(T.bb.lo.z), ref[0]);
    F.bihhdr[3 * hdr + 1] = mk4u(round_up(T.bb.hi.x), round_up(T.bb.hi.y), round_up(T.bb.hi.z), cls);
    // (x: the records-to-pool delta of a triangle or sphere tree, y / z: the packet walk's root and flag, a triangle tree's -- emit_leaf_bih;
    // w: the tree's depth -- the generic tier walks a tree as a packet when its per-wave stack holds it -- and, in bit 31, whether
    // every item is answered in place: kBihItemsInPlace)
    in_place = in_place && !T.nodes.empty() && !T.nodes[0].leaf;
    F.bihhdr[3 * hdr + 2] = F4{as_float_bits(0u), as_float_bits(0u), as_float_bits(0u), as_float_bits((uint32_t)T.depth | (in_place ? kBihItemsInPlace : 0u))};
    if (in_place) F.max_sphere_bih_depth = std::max(F.max_sphere_bih_depth, T.depth);
    if (has_inst) {
      movable_bihs.insert(id);
      InstBihInfo B;
      B.node = id; B.hdr = hdr; B.first_slot = base; B.n_slots = nslots;
      B.first_rec = item_recs.front(); B.rec_span = item_recs.back() + 1u - B.first_rec;  // (records only ever grow: the first item's is the lowest)
      B.child_bound.assign(6 * item_ids.size(), 0.0);
      box6(T.bb, B.bound6);
      for (size_t j = 0; j < item_ids.size(); j++) {
        B.rec_off.push_back(item_recs[j] - B.first_rec);
        const Box3 b = G.bound(item_ids[j]);
        int live_obj = -1;
        B.kind.push_back(item_kind(item_ids[j], live_obj));
        B.live.push_back(live_obj);
        B.xf_at.push_back(-1);
        B.box64.resize(B.box64.size() + 6);
        box6(b, &B.box64[B.box64.size() - 6]);
        B.rows.push_back(F4{round_down((b.lo.x - kDelta)), round_down((b.lo.y - kDelta)), round_down((b.lo.z - kDelta)), 0.0f});
        B.rows.push_back(F4{round_up((b.hi.x + kDelta)), round_up((b.hi.y + kDelta)), round_up((b.hi.z + kDelta)), 0.0f});
        B.rows.push_back(F4{round_down(b.lo.x), round_down(b.lo.y), round_down(b.lo.z), 0.0f});
        B.rows.push_back(F4{round_up(b.hi.x), round_up(b.hi.y), round_up(b.hi.z), 0.0f});
        const int inst = G.peel_wrappers(item_ids[j]);
        if (G.at(inst).kind != K_INSTANCE) continue;
        const Box3 cb = G.bound(G.at(inst).a);
        const double c6[6] = {cb.lo.x, cb.lo.y, cb.lo.z, cb.hi.x, cb.hi.y, cb.hi.z};
        std::copy(c6, c6 + 6, B.child_bound.begin() + 6 * (ptrdiff_t)j);
        inst_items.push_back({inst, id, (uint32_t)j});
        if (B.kind.back() == InstBihInfo::kInstancedLive) {
          const Xf& x = G.at(inst).xf;
          B.xf_at.back() = (int32_t)(B.live_xf.size() / 24);
          B.live_xf.insert(B.live_xf.end(), x.f.m, x.f.m + 12);
          B.live_xf.insert(B.live_xf.end(), x.i.m, x.i.m + 12);
        }
      }
      tree_levels(T.nodes, [&](size_t k) { return base + slot[k]; }, B.level_nodes, B.level_off);
      F.inst_bihs.push_back(std::move(B));
    }
    return U4{R_BIH, hdr, 0, (uint32_t)n.uid};
  }
  static void box6(const Box3& b, double* o) { o[0] = b.lo.x; o[1] = b.lo.y; o[2] = b.lo.z; o[3] = b.hi.x; o[4] = b.hi.y; o[5] = b.hi.z; }
  // An item of a bih by what a refit makes of it (InstBihInfo::ItemKind); live: the Mesh or Bih it hangs on
  uint8_t item_kind(int item, int& live) const {
    live = -1;
    const int z = G.peel_wrappers(item);
    const int k = G.at(z).kind;
    if (can_move(z)) { live = z; return InstBihInfo::kDirectLive; }
    if (k != K_INSTANCE) return InstBihInfo::kStatic;
    const int c = G.peel_wrappers(G.at(z).a);
    if (can_move(c)) { live = c; return InstBihInfo::kInstancedLive; }
    return InstBihInfo::kInstance;
  }
  // a Mesh, or a Bih that has update tables of its own -- a triangle bih, a sphere bih, a bih with Instance or live items -- which emit_bih
  // has made by the time a parent asks (an item is emitted before its kind is looked at).  A bih of boxes, say, never changes: static.
  bool can_move(int id) const { return G.at(id).kind == K_MESH || (G.at(id).kind == K_BIH && movable_bihs.count(id) != 0); }
  std::set<int> movable_bihs;
  struct InstItem { int inst, bih; uint32_t item; };
  std::vector<InstItem> inst_items;  // every (Instance, bih, item) emit_bih met: bound to F.inst_updates by mark_updatable

  U4 emit_mesh(const Node& n, int id) {
    const MeshData& M = *n.mesh;
    F.max_mesh_depth = std::max(F.max_mesh_depth, M.depth);
    uint32_t hdr = (uint32_t)(F.meshhdr.size() / 2);
    uint32_t nbase = (uint32_t)(F.meshnodes.size() / 4);
    MeshUpdateInfo U;
    U.node = id; U.nv = (int)M.verts.size(); U.nn = (int)M.norms.size(); U.hdr = hdr; U.first_node = nbase; U.first_tri = (uint32_t)(F.mtris.size() / 3);
    // node index remap: branches only (leaves are encoded in the parent's ref)
    std::vector<uint32_t> bidx(M.nodes.size(), 0);
    uint32_t nb = 0;
    for (size_t k = 0; k < M.nodes.size(); k++) if (!M.nodes[k].leaf) bidx[k] = nbase + nb++;
    F.meshnodes.resize((size_t)4 * (nbase + nb));
    std::vector<uint32_t> ref(M.nodes.size(), 0);
    // leaves first (preorder), so triangle runs follow traversal order
    for (size_t k = 0; k < M.nodes.size(); k++) {
      const MeshData::Node& mn = M.nodes[k];
      if (!mn.leaf) { ref[k] = bidx[k]; continue; }
      uint32_t first = (uint32_t)(F.mtris.size() / 3), count = (uint32_t)mn.tris.size();
      if (first + count >= (1u << 27)) throw limit_error("mesh has too many triangles");
      for (size_t q = 0; q < mn.tris.size(); q++) {
        const MeshTri& t = M.tris[mn.tris[q]];
        const D3 &a = M.verts[t.a], &b = M.verts[t.b], &c = M.verts[t.c];
        D3 e1 = b - a, e2 = c - a, nn = normalize(cross(e1, e2));
        F.mtris.push_back(mk4(a.x, a.y, a.z, nn.x));
        F.mtris.push_back(mk4(e1.x, e1.y, e1.z, nn.y));
        F.mtris.push_back(mk4(e2.x, e2.y, e2.z, nn.z));
        U4 meta{0, 0, q == 0 ? count : 0u, 0};
        const int32_t row[8] = {t.a, t.b, t.c, t.na, t.nb, t.nc, t.na != -1 ? (int32_t)F.trinorms.size() : -1, 0};
        U.rows.insert(U.rows.end(), row, row + 8);
        if (t.na != -1) {
          meta.x = (uint32_t)F.trinorms.size() + 1;
          for (int ni : {t.na, t.nb, t.nc}) F.trinorms.push_back(mk4(M.norms[ni].x, M.norms[ni].y, M.norms[ni].z, 0));
        }
        if (t.tex != -1) meta.y = (uint32_t)M.mats[t.tex] + 1;
        F.mtrimeta.push_back(meta);
      }
      if (count == 0) {  // keep `first` addressable
        F.mtrimeta.push_back(U4{0, 0, 0, 0}); for (int q = 0; q < 3; q++) F.mtris.push_back(F4{0, 0, 0, 0});
        const int32_t row[8] = {-1, -1, -1, -1, -1, -1, -1, 0};
        U.rows.insert(U.rows.end(), row, row + 8);
      }
      ref[k] = 0x80000000u | ((count >= 15 ? 15u : count) << 27) | first;
    }
    for (size_t k = 0; k < M.nodes.size(); k++) {
      const MeshData::Node& mn = M.nodes[k];
      if (mn.leaf) continue;
      F4* o = &F.meshnodes[(size_t)4 * bidx[k]];
      // boxes rounded outward
      o[0] = mk4u(round_down(mn.lbb.lo.x), round_down(mn.lbb.lo.y), round_down(mn.lbb.lo.z), ref[mn.left]);
      o[1] = mk4(round_up(mn.lbb.hi.x), round_up(mn.lbb.hi.y), round_up(mn.lbb.hi.z), 0);
      o[2] = mk4u(round_down(mn.rbb.lo.x), round_down(mn.rbb.lo.y), round_down(mn.rbb.lo.z), ref[mn.right]);
      o[3] = mk4(round_up(mn.rbb.hi.x), round_up(mn.rbb.hi.y), round_up(mn.rbb.hi.z), 0);
    }
    F.meshhdr.push_back(mk4u(round_down(M.bb.lo.x), round_down(M.bb.lo.y), round_down(M.bb.lo.z), ref[0]));
    F.meshhdr.push_back(mk4(round_up(M.bb.hi.x), round_up(M.bb.hi.y), round_up(M.bb.hi.z), 0));
    U.n_nodes = nb; U.n_tris = (uint32_t)(F.mtris.size() / 3) - U.first_tri;
    box6(M.bb, U.bound6);
    tree_levels(M.nodes, [&](size_t k) { return bidx[k]; }, U.level_nodes, U.level_off);
    F.mesh_updates.push_back(std::move(U));
    return U4{R_MESH, hdr, 0, (uint32_t)n.uid};
  }

  // ---- flat tier root program ----
  // Walk Tex / Tag / flag wrappers and lists from the root; every leaf of that walk must be a simple primitive,
  // a homogeneous BIH or a mesh.  `incoming` = texture stack pushed by the wrappers above the entry.
  void collect_entries(int id, uint32_t incoming, int nin, uint32_t flags) {
    if (F.tier != 0) return;
    const Node& n = G.at(id);
    switch (n.kind) {
      case K_VOID: return;
      case K_TAG: collect_entries(n.a, incoming, nin, flags); return;
      case K_NOSHADOW: collect_entries(n.a, incoming, nin, flags | RF_NOSHADOW); return;
      case K_ONLYSHADOW: collect_entries(n.a, incoming, nin, flags | RF_NOVIS); return;
      case K_TEX:
        if (nin >= 2) { F.tier = 1; F.why_generic = "more than two Tex levels above a root entry"; return; }
        // `tex:texs`: the inner Tex is pushed later, so it sits in front
        collect_entries(n.a, (incoming << 16) | (uint32_t)(n.mat + 1), nin + 1, flags);
        return;
      case K_LIST: for (int k : n.kids) collect_entries(k, incoming, nin, flags); return;
      case K_BIH: {
        U4 r = emit(id);
        uint32_t cls;
        std::memcpy(&cls, &F.bihhdr[3 * r.y + 1].w, 4);
        if (cls == BC_GENERIC) { F.tier = 1; F.why_generic = "BIH with composite items"; return; }
        F.entries.push_back(U4{slot(r), incoming, flags, 0});
        return;
      }
      case K_MESH: F.entries.push_back(U4{slot(emit(id)), incoming, flags, 0}); return;
      default:
        if (is_prim(n.kind) && n.kind != K_CYL && n.kind != K_CONE) { F.entries.push_back(U4{slot(emit(id)), incoming, flags, 0}); return; }
        if (csg_simple(id)) { F.entries.push_back(U4{slot(emit(id)), incoming, flags, 0}); return; }  // a Difference / Intersection / Instance over primitives
        F.tier = 1; F.why_generic = std::string("root reaches a ") + kind_name(n.kind);
        return;
    }
  }
};

}  // namespace glome
